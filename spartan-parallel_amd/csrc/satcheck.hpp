// spg — R1CS satisfiability on the device (satcheck.hip): Az[i] Bz[i] == Cz[i] for every row of three ragged
// (p, q_rev, 0, x_rev) tables of one shape, the check of the reference's R1CSInstance::is_sat
// (src/r1csinstance.rs:322-357) over the tables multiply_vec_block leaves in HBM. Here the host-only part: the
// table descriptors, the decoding of the kernel's key, the shape check every entry makes before a launch, and the
// merge of the ranks' reports (libspg_hostcheck.so's spgh_sat_merge runs it without a GPU).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../include/spg.h"

struct spg_ctx;

namespace spg {

struct Fq;

// instance p of the flat domain: 2^lg_q x 2^lg_rows rows stored at [dom_off, dom_off + 2^(lg_q + lg_rows)), the row
// (q, x) at dom_off + brev(q) 2^lg_rows + brev(x). Its natural key is dom_off + q 2^lg_rows + x: keys order rows as
// (p, q, row) does, p in table order.
struct SatDesc {
  uint64_t dom_off;
  uint32_t lg_q, lg_rows;
};
static const int kSatMaxP = 32;  // descriptors in the kernel arguments (pqx.hpp kMaxP); more go to device memory
struct SatArgs {
  int P;
  const SatDesc* ext;  // more than kSatMaxP instances: every descriptor in device memory (else null)
  SatDesc in[kSatMaxP];
};

static const uint64_t kSatNoKey = ~0ULL;
// what the kernel leaves: violating rows, the lowest natural key among them (kSatNoKey: none)
struct SatRecord {
  uint64_t count, key;
};

inline uint32_t sat_brev(uint32_t v, uint32_t lg) {
  uint32_t r = 0;
  for (uint32_t i = 0; i < lg; i++) r |= ((v >> i) & 1u) << (lg - 1 - i);
  return r;
}

// the descriptors of a packed table: instance p holds num_proofs[p] x num_cons[p] rows (powers of two), one after
// another. nullptr, or what is wrong with the shape (nothing is launched then). Every position a descriptor decodes
// to lies below *total = sum_p num_proofs[p] num_cons[p], the tables' allocation.
inline const char* sat_descs(const size_t* num_proofs, const size_t* num_cons, size_t P, std::vector<SatDesc>* out,
                             uint64_t* total) {
  auto lg = [](size_t v) {
    uint32_t k = 0;
    while (((size_t)1 << k) < v) k++;
    return k;
  };
  out->clear();
  uint64_t off = 0;
  if (P >= 0x7fffffffULL) return "too many instances";
  for (size_t p = 0; p < P; p++) {
    const size_t q = num_proofs[p], x = num_cons[p];
    if (!q || (q & (q - 1)) || !x || (x & (x - 1))) return "num_proofs and num_cons must be powers of two";
    if (q > ((size_t)1 << 31) || x > ((size_t)1 << 31)) return "an instance is too large";
    out->push_back(SatDesc{off, lg(q), lg(x)});
    off += (uint64_t)q * x;
    if (off >= ((uint64_t)1 << 40)) return "more than 2^40 rows";
  }
  *total = off;
  return nullptr;
}

// key -> (p, q, row) and the stored position of that row
inline void sat_decode(const std::vector<SatDesc>& d, uint64_t key, uint64_t* p, uint64_t* q, uint64_t* row,
                       uint64_t* stored) {
  size_t lo = 0, hi = d.size() - 1;
  while (lo < hi) {
    const size_t mid = (lo + hi + 1) >> 1;
    if (d[mid].dom_off <= key) lo = mid;
    else hi = mid - 1;
  }
  const uint64_t loc = key - d[lo].dom_off;
  *p = lo;
  *q = loc >> d[lo].lg_rows;
  *row = loc & (((uint64_t)1 << d[lo].lg_rows) - 1);
  *stored = d[lo].dom_off + ((uint64_t)sat_brev((uint32_t)*q, d[lo].lg_q) << d[lo].lg_rows) +
            sat_brev((uint32_t)*row, d[lo].lg_rows);
}

// the ranks' reports (each with p already the caller's instance index) -> the report every rank returns: rows and
// violations summed, and (p, q, row, az, bz, cz) of the lowest (p, q, row) among the ranks that saw a violation
inline void sat_merge(const spg_sat_report* r, int nranks, spg_sat_report* out) {
  memset(out, 0, sizeof(*out));
  const spg_sat_report* best = nullptr;
  for (int k = 0; k < nranks; k++) {
    out->rows += r[k].rows;
    out->violations += r[k].violations;
    if (!r[k].violations) continue;
    if (!best || r[k].p < best->p || (r[k].p == best->p && (r[k].q < best->q || (r[k].q == best->q && r[k].row < best->row))))
      best = &r[k];
  }
  if (!best) return;
  out->p = best->p;
  out->q = best->q;
  out->row = best->row;
  memcpy(out->az, best->az, sizeof(out->az));
  memcpy(out->bz, best->bz, sizeof(out->bz));
  memcpy(out->cz, best->cz, sizeof(out->cz));
}

// "R1CS unsatisfied: instance P execution Q constraint R (V of N rows)"
inline std::string sat_message(const spg_sat_report& r) {
  return "R1CS unsatisfied: instance " + std::to_string(r.p) + " execution " + std::to_string(r.q) + " constraint " +
         std::to_string(r.row) + " (" + std::to_string(r.violations) + " of " + std::to_string(r.rows) + " rows)";
}

// (satcheck.hip) one k_sat_check launch over the three tables (device pointers, *total elements each as sat_descs
// gave it), the record read back, and the three values at the lowest violating row when there is one. out->p is the
// position in d. Synchronous.
int sat_check_run(spg_ctx* ctx, const std::vector<SatDesc>& d, uint64_t total, const Fq* Az, const Fq* Bz,
                  const Fq* Cz, spg_sat_report* out);

}  // namespace spg
