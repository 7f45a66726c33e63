// spg — many short group equations sum_i s_i P_i = identity in one call (spg_eqs_check, eqcheck.hip): the host-only
// part. A call is one flat list of T terms cut into E consecutive equations by first[0 .. E]; a term is a Montgomery
// scalar and a point in one of three operand forms (a reference into the call's compressed pool, its extended pool or
// the caller's resident base points). Here: the argument check every entry makes before anything is launched, the
// launch plan, and the host evaluation of a term list with hcurve.hpp (libspg_hostcheck.so's spgh_eqs_check, the
// semantics of the device entry without a GPU).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "hcurve.hpp"

struct spg_ctx;

namespace spg {

enum : uint8_t { kEqsCompressed = 0, kEqsExtended = 1, kEqsIndex = 2 };  // SPG_EQS_* of spg.h
enum : uint8_t { kEqsIdentity = 0, kEqsNonzero = 1, kEqsBadPoint = 2 };

struct EqsView {
  const uint8_t* kinds = nullptr;     // T operand forms
  const uint32_t* refs = nullptr;     // T indices into the pool of the term's form
  const Fq* scalars = nullptr;        // T Montgomery scalars
  const size_t* first = nullptr;      // E + 1 term offsets, first[0] = 0, first[E] = T
  size_t E = 0;
  const uint8_t* compressed = nullptr;  // nc x 32
  size_t nc = 0;
  const uint8_t* extended = nullptr;    // ne x 128 (X, Y, Z, T; spg_msm_partial layout)
  size_t ne = 0;
  size_t nb = 0;                        // points of the base handle (0: none)
  size_t T() const { return E ? first[E] : 0; }
};

// nullptr for a well-formed call, else what is wrong with it (SPG_E_ARG, nothing launched)
inline const char* eqs_validate(const EqsView& v) {
  if (!v.E) return nullptr;
  if (!v.first) return "first is null";
  if (v.first[0] != 0) return "first[0] must be 0";
  for (size_t e = 0; e < v.E; e++)
    if (v.first[e + 1] < v.first[e]) return "first must be non-decreasing";
  const size_t T = v.first[v.E];
  if (T >= 0x7fffffffULL || v.E >= 0x7fffffffULL) return "too many terms";
  if (T && (!v.kinds || !v.refs || !v.scalars)) return "terms are null";
  if ((v.nc && !v.compressed) || (v.ne && !v.extended)) return "operand pool is null";
  for (size_t i = 0; i < T; i++) {
    if (v.kinds[i] > kEqsIndex) return "unknown operand form";
    const size_t lim = v.kinds[i] == kEqsCompressed ? v.nc : v.kinds[i] == kEqsExtended ? v.ne : v.nb;
    if (v.refs[i] >= lim) return "operand index past its pool";
  }
  return nullptr;
}

// launch plan: the term kernel runs one lane per term in workgroups of one wavefront (a proof's few thousand terms
// spread over as many CUs as they fill wavefronts); the sum kernel one wavefront per equation, four per workgroup
constexpr int kEqsTermBS = 64;
constexpr int kEqsSumBS = 256;
constexpr int kEqsSumPerWG = kEqsSumBS / 64;
struct EqsPlan {
  unsigned term_grid, sum_grid;
};
inline EqsPlan eqs_plan(size_t T, size_t E) {
  return EqsPlan{(unsigned)((T + kEqsTermBS - 1) / kEqsTermBS), (unsigned)((E + kEqsSumPerWG - 1) / kEqsSumPerWG)};
}

// the entry behind spg_eqs_check and the verifiers' deferred mode (eqcheck.hip): v is validated there; base = v.nb
// affine Niels points on the device (an spg_points' or a generator set's). Synchronous.
int eqs_check_run(spg_ctx* ctx, const EqsView& v, const Niels* base, uint8_t* sums, uint8_t* status, long* bad_term);

// an HExt as the 128 bytes of the extended operand form
inline void eqs_ext_bytes(const h::HExt& P, uint8_t out[128]) {
  h::fe_to_bytes(P.X, out);
  h::fe_to_bytes(P.Y, out + 32);
  h::fe_to_bytes(P.Z, out + 64);
  h::fe_to_bytes(P.T, out + 96);
}
inline h::HExt eqs_ext_from_bytes(const uint8_t in[128]) {
  Ext P;
  memcpy(&P, in, 128);
  return h::hext_from_dev(P);
}

// The host evaluation (v validated): base = the nb base points' encodings. sums (optional) E x 32, status E bytes,
// *bad_term (optional) the lowest term whose encoding DECODE rejects, else -1. A rejected base encoding counts as a
// rejected term.
inline void eqs_host_eval(const EqsView& v, const uint8_t* base, uint8_t* sums, uint8_t* status, long* bad_term) {
  long bad = -1;
  for (size_t e = 0; e < v.E; e++) {
    h::HExt acc = h::hext_identity();
    bool rejected = false;
    for (size_t i = v.first[e]; i < v.first[e + 1]; i++) {
      h::HExt P;
      bool ok = true;
      if (v.kinds[i] == kEqsCompressed)
        ok = h::hext_decompress(v.compressed + 32 * (size_t)v.refs[i], P);
      else if (v.kinds[i] == kEqsExtended)
        P = eqs_ext_from_bytes(v.extended + 128 * (size_t)v.refs[i]);
      else
        ok = h::hext_decompress(base + 32 * (size_t)v.refs[i], P);
      if (!ok) {
        if (bad < 0) bad = (long)i;
        rejected = true;
        continue;
      }
      const Fq k = fq_from_mont(v.scalars[i]);  // Scalar::to_bytes
      uint8_t b[32];
      for (int w = 0; w < 8; w++)
        for (int j = 0; j < 4; j++) b[4 * w + j] = (uint8_t)(k.l[w] >> (8 * j));
      acc = h::hext_add(acc, h::hext_scalar_mul(P, b));
    }
    // the ristretto255 identity (RFC 9496 4.3.3 against (0, 1)): X = 0 or Y = 0
    status[e] = rejected ? kEqsBadPoint : (h::fe_is_zero(acc.X) || h::fe_is_zero(acc.Y)) ? kEqsIdentity : kEqsNonzero;
    if (sums) {
      if (rejected)
        memset(sums + 32 * e, 0, 32);
      else
        h::hext_compress(acc, sums + 32 * e);
    }
  }
  if (bad_term) *bad_term = bad;
}

}  // namespace spg
