// spg — host build of the product's field / curve / transcript code (the same headers the HIP kernels
// compile), exported for the CPU test suite so the arithmetic can be checked against the oracle
// without a GPU. Not part of the proving path.
#include <stdio.h>
#include <string.h>

#include <vector>

#include <atomic>
#include <memory>
#include <random>

#include "comm.hpp"
#include "curve.hpp"
#include "eqcheck.hpp"
#include "hcurve.hpp"
#include "hvec.hpp"
#include "hostmath.hpp"
#include "hpool.hpp"
#include "keccak.hpp"
#include "knobs.hpp"
#include "msm_plan.hpp"
#include "pe_plan.hpp"
#include "r1cs_desc.hpp"
#include "satcheck.hpp"
#include "snark_shape.hpp"
#include "spark_shape.hpp"
#include "vmsm.hpp"
#include "ws_slots.hpp"

using namespace spg;

static Fq ldq(const uint64_t* p) { Fq a; memcpy(a.l, p, 32); return a; }
static void stq(uint64_t* p, const Fq& a) { memcpy(p, a.l, 32); }

extern "C" {

// op: 0 add, 1 sub, 2 mul, 3 neg, 4 square, 5 invert, 6 from_mont, 7 to_mont, 8 mul_ps, 9 mul32
void spgh_fq_op(int op, const uint64_t* a, const uint64_t* b, uint64_t* out, size_t n) {
  for (size_t i = 0; i < n; i++) {
    Fq x = ldq(a + 4 * i), y = b ? ldq(b + 4 * i) : fq_zero(), r;
    switch (op) {
      case 0: r = fq_add(x, y); break;
      case 1: r = fq_sub(x, y); break;
      case 2: r = fq_mul(x, y); break;
      case 3: r = fq_neg(x); break;
      case 4: r = fq_sqr(x); break;
      case 5: r = fq_inv(x); break;
      case 6: r = fq_from_mont(x); break;
      case 8: r = fq_mul_ps(x, y); break;  // the device's product-scanning Montgomery product
      case 9: r = fq_mul32(x, y); break;   // the CIOS form
      default: r = fq_to_mont(x); break;
    }
    stq(out + 4 * i, r);
  }
}

// op: 0 add, 1 sub, 2 mul, 3 sqr, 4 inv, 5 canon, 6 mul (device product scanning), 7 sqr (device),
// 12 mul_k (k = b's low 18 bits); raw (not canonicalised) outputs: 8 addsub(+), 9 addsub(-), 10 add, 11 sub;
// inputs/outputs as 8 x u32 (loose allowed)
void spgh_fp_op(int op, const uint32_t* a, const uint32_t* b, uint32_t* out, size_t n) {
  for (size_t i = 0; i < n; i++) {
    Fp x, y, r;
    memcpy(x.l, a + 8 * i, 32);
    if (b) memcpy(y.l, b + 8 * i, 32); else y = fp_zero();
    switch (op) {
      case 0: r = fp_add(x, y); break;
      case 1: r = fp_sub(x, y); break;
      case 2: r = fp_mul(x, y); break;
      case 3: r = fp_sqr(x); break;
      case 4: r = fp_inv(x); break;
      case 6: r = fp_mul_ps(x, y); break;
      case 7: r = fp_sqr_ps(x); break;
      case 8: r = fp_addsub(x, y, false); break;
      case 9: r = fp_addsub(x, y, true); break;
      case 10: r = fp_add(x, y); break;
      case 11: r = fp_sub(x, y); break;
      case 12: r = fp_mul_k(x, y.l[0] & 0x3ffffu); break;
      default: r = x; break;
    }
    if (op < 8 || op > 11) r = fp_canon(r);
    memcpy(out + 8 * i, r.l, 32);
  }
}

void spgh_from_uniform(const uint8_t* b64, uint8_t* out, size_t n) {
  for (size_t i = 0; i < n; i++) ext_compress(ristretto_from_uniform_bytes(b64 + 64 * i), out + 32 * i);
}
int spgh_roundtrip(const uint8_t* in, uint8_t* out) {
  Ext p;
  if (!ext_decompress(in, p)) return 0;
  ext_compress(p, out);
  return 1;
}
// the same round trip through the host's radix-2^51 decoder (hcurve.hpp), the one the verifier and proto.hip use
int spgh_hext_roundtrip(const uint8_t* in, uint8_t* out) {
  h::HExt p;
  if (!h::hext_decompress(in, p)) return 0;
  h::hext_compress(p, out);
  return 1;
}
// op: 0 add, 1 double, 2 madd via niels, 3 madd negated
int spgh_point_op(int op, const uint8_t* a, const uint8_t* b, uint8_t* out) {
  Ext p, q;
  if (!ext_decompress(a, p)) return 0;
  if (op != 1 && !ext_decompress(b, q)) return 0;
  Ext r;
  switch (op) {
    case 0: r = ext_add(p, q); break;
    case 1: r = ext_dbl(p); break;
    case 2: r = ext_madd(p, ext_to_niels(q), false); break;
    default: r = ext_madd(p, ext_to_niels(q), true); break;
  }
  ext_compress(r, out);
  return 1;
}
int spgh_niels_roundtrip(const uint8_t* a, uint8_t* out) {
  Ext p;
  if (!ext_decompress(a, p)) return 0;
  ext_compress(niels_to_ext(ext_to_niels(p)), out);
  return 1;
}
void spgh_shake256(const uint8_t* in, size_t n, uint8_t* out, size_t m) {
  Shake256 s;
  s.update(in, n);
  s.read(out, m);
}
void spgh_merlin_simple(const char* label, const char* l1, const uint8_t* m1, size_t m1n, const char* l2,
                        uint8_t* out, size_t m) {
  Merlin t(label);
  t.message(l1, m1, m1n);
  t.challenge(l2, out, m);
}

// A caller-owned merlin::Transcript behind spg_transcript_new_callbacks, in native code: what the Rust caller's
// `extern "C"` trampolines over `&mut Transcript` do (src/lib.rs:1022). The two
// callbacks have the spg_transcript_append_fn / spg_transcript_challenge_fn signatures and take the Merlin as `user`,
// so bench.py can time a prove in the drop-in mode with no Python on the transcript path.
void* spgh_merlin_new(const char* label) { return new Merlin(label); }
void spgh_merlin_free(void* t) { delete static_cast<Merlin*>(t); }
int spgh_merlin_append_cb(void* user, const char* label, const uint8_t* msg, size_t len) {
  static_cast<Merlin*>(user)->message(label, msg, len);
  return 0;
}
int spgh_merlin_challenge_cb(void* user, const char* label, uint8_t* out, size_t len) {
  static_cast<Merlin*>(user)->challenge(label, out, len);
  return 0;
}

// Host radix-2^51 curve (hcurve.hpp) against the device-form curve on the same inputs: for n uniform
// 64-byte strings, P_i = from_uniform_bytes; checks compress, decompress->compress, add, dbl, mixed add
// through batch-normalised Niels, and scalar multiplication by the 32-byte scalars k. Returns the
// number of mismatches.
int spgh_hcurve_check(const uint8_t* uni, const uint8_t* k, size_t n) {
  using namespace spg;
  int bad = 0;
  std::vector<Ext> P(n);
  std::vector<h::HExt> H(n);
  for (size_t i = 0; i < n; i++) {
    P[i] = ristretto_from_uniform_bytes(uni + 64 * i);
    H[i] = h::hext_from_dev(P[i]);
  }
  std::vector<h::HNiels> N;
  h::hext_batch_to_niels(H, N);
  for (size_t i = 0; i < n; i++) {
    uint8_t a[32], b[32];
    ext_compress(P[i], a);
    h::hext_compress(H[i], b);
    bad += memcmp(a, b, 32) != 0;
    h::HExt D;
    bad += !h::hext_decompress(a, D);
    h::hext_compress(D, b);
    bad += memcmp(a, b, 32) != 0;
    size_t j = (i + 1) % n;
    ext_compress(ext_add(P[i], P[j]), a);
    h::hext_compress(h::hext_add(H[i], H[j]), b);
    bad += memcmp(a, b, 32) != 0;
    h::hext_compress(h::hext_madd(H[i], N[j]), b);
    bad += memcmp(a, b, 32) != 0;
    ext_compress(ext_dbl(P[i]), a);
    h::hext_compress(h::hext_dbl(H[i]), b);
    bad += memcmp(a, b, 32) != 0;
    uint32_t kk[8];
    for (int w = 0; w < 8; w++)
      kk[w] = (uint32_t)k[32 * i + 4 * w] | ((uint32_t)k[32 * i + 4 * w + 1] << 8) |
              ((uint32_t)k[32 * i + 4 * w + 2] << 16) | ((uint32_t)k[32 * i + 4 * w + 3] << 24);
    ext_compress(ext_scalar_mul(P[i], kk), a);
    h::hext_compress(h::hext_scalar_mul(H[i], k + 32 * i), b);
    bad += memcmp(a, b, 32) != 0;
  }
  uint8_t bad_enc[32];
  memset(bad_enc, 0xff, 32);
  h::HExt X;
  bad += h::hext_decompress(bad_enc, X);  // non-canonical must be rejected
  return bad;
}

// The 8-lane IFMA sums (hvec.hpp) against the scalar additions: for m = 0 .. n entries, the sum of the first m Niels
// forms (mixed additions) and of the first m extended points (full additions), compared by encoding. Returns the
// number of mismatches, or -1 when this CPU has no AVX-512 IFMA (nothing to check).
int spgh_vec_check(const uint8_t* uni, size_t n) {
  using namespace spg;
  if (!h::ifma_on()) return -1;
  int bad = 0;
  std::vector<h::HExt> H(n);
  for (size_t i = 0; i < n; i++) H[i] = h::hext_from_dev(ristretto_from_uniform_bytes(uni + 64 * i));
  std::vector<h::HNiels> N;
  h::hext_batch_to_niels(H, N);
  std::vector<const h::HNiels*> ptr(n);
  for (size_t i = 0; i < n; i++) ptr[i] = &N[i];
  h::HExt s1 = h::hext_identity(), s2 = h::hext_identity();
  for (size_t m = 0; m <= n; m++) {
    if (m) {
      s1 = h::hext_madd(s1, N[m - 1]);
      s2 = h::hext_add(s2, H[m - 1]);
    }
    uint8_t a[32], b[32];
    h::hext_compress(s1, a);
    h::hext_compress(h::niels_sum8(ptr.data(), m), b);
    bad += memcmp(a, b, 32) != 0;
    h::hext_compress(s2, a);
    h::hext_compress(h::ext_sum8(H.data(), m), b);
    bad += memcmp(a, b, 32) != 0;
  }
  return bad;
}

// The batched encoding of doubles (hcurve.hpp, hext_double_and_compress_batch) against the lone encoding of 2 Q, over
// n hash-to-group points, each also moved by the 2- and 4-torsion points, and the identity and the torsion points
// themselves (zero e g f h). Returns the mismatches (0), or -1 for n == 0.
int spgh_dbl_compress_check(const uint8_t* uni, size_t n) {
  using namespace spg;
  if (!n) return -1;
  const h::HExt T2{h::fe_zero(), h::fe_neg(h::fe_one()), h::fe_one(), h::fe_zero()};
  const h::HExt T4{h::K().sqrt_m1, h::fe_zero(), h::fe_one(), h::fe_zero()};
  std::vector<h::HExt> Q;
  for (size_t i = 0; i < n; i++) {
    const h::HExt P = h::hext_from_dev(ristretto_from_uniform_bytes(uni + 64 * i));
    Q.push_back(P);
    Q.push_back(h::hext_add(P, T2));
    Q.push_back(h::hext_add(P, T4));
    if (i == n / 2) {
      Q.push_back(h::hext_identity());
      Q.push_back(T2);
      Q.push_back(T4);
    }
  }
  std::vector<uint8_t> got(32 * Q.size());
  h::hext_double_and_compress_batch(Q.data(), Q.size(), (uint8_t(*)[32])got.data());
  std::vector<uint8_t> got8(32 * Q.size());
  const bool vec = h::ifma_on();
  if (vec) h::double_and_compress_batch8(Q.data(), Q.size(), (uint8_t(*)[32])got8.data());
  int bad = 0;
  for (size_t i = 0; i < Q.size(); i++) {
    uint8_t want[32];
    h::hext_compress(h::hext_dbl(Q[i]), want);
    bad += memcmp(want, got.data() + 32 * i, 32) != 0;
    if (vec) bad += memcmp(want, got8.data() + 32 * i, 32) != 0;
  }
  // every length 1 .. 20 through the 8-lane form (partial groups)
  for (size_t m = 1; vec && m <= 20 && m <= Q.size(); m++) {
    h::double_and_compress_batch8(Q.data(), m, (uint8_t(*)[32])got8.data());
    for (size_t i = 0; i < m; i++) bad += memcmp(got.data() + 32 * i, got8.data() + 32 * i, 32) != 0;
  }
  return bad;
}

// The cross-rank exchange of every sharded call (comm.hpp: api.hip's comm_sum_fq, which Prover::sum_ranks -- the R1CS
// prover's p1_round_single / p2_round_single -- and the SPARK / multi_evaluate shards use): gather every rank's status and n partial scalars through the caller's
// allgather and sum them mod q. Returns the transport's error (-1), else the first non-zero status of any rank
// (so a failing rank fails every rank alike), else 0 with out = the sums.
int spgh_comm_sum(spg_allgather_fn fn, void* user, int nranks, int status, const uint64_t* mine, size_t n,
                  uint64_t* out) {
  std::vector<Fq> v(n);
  for (size_t i = 0; i < n; i++) v[i] = ldq(mine + 4 * i);
  std::vector<uint8_t> all;
  int64_t first = 0;
  if (allgather_with_status(fn, user, nranks, status, v.data(), n * sizeof(Fq), all, &first) != 0) return -1;
  if (first) return (int)first;
  sum_over_ranks(all.data(), nranks, n, v.data());
  for (size_t i = 0; i < n; i++) stq(out + 4 * i, v[i]);
  return 0;
}

// the prover's host scalar helpers (hostmath.hpp): UniPoly::from_evals of degree 3 -> coeffs[4] and evaluate(r)
void spgh_uni_from_evals3(const uint64_t* evals, const uint64_t* r, uint64_t* coeffs, uint64_t* at_r) {
  Fq e[4];
  for (int i = 0; i < 4; i++) e[i] = ldq(evals + 4 * i);
  FqV c = uni_from_evals3(e);
  for (int i = 0; i < 4; i++) stq(coeffs + 4 * i, c[i]);
  stq(at_r, uni_eval(c, ldq(r)));
}
// DensePolynomial::evaluate of n host scalars at r (ell scalars) and EqPolynomial::evals(r) (2^ell scalars)
void spgh_dense_eval(const uint64_t* Z, size_t n, const uint64_t* r, size_t ell, uint64_t* out, uint64_t* chis) {
  FqV z(n), rv(ell);
  for (size_t i = 0; i < n; i++) z[i] = ldq(Z + 4 * i);
  for (size_t i = 0; i < ell; i++) rv[i] = ldq(r + 4 * i);
  stq(out, dense_eval_host(z, rv));
  FqV e = eq_evals_host(rv);
  for (size_t i = 0; i < e.size(); i++) stq(chis + 4 * i, e[i]);
}

// The host pool (hpool.hpp) under stress: `bursts` parallel_for calls of random size 1..max_n on a fresh
// pool of `workers` threads whose workers sleep `delay_us` between their generation and function loads
// and whose caller sleeps `delay_us` between publishing a burst's function/count and opening it (the two
// sides of the stale-snapshot race window). Every task bumps its own counter; right after each call
// returns, every counter must be exactly 1 and no task may still be running. Returns the number of
// violations (0 = pass).
long spgh_pool_stress(int workers, int bursts, int max_n, int delay_us, unsigned seed) {
  spg::Pool pool(workers, delay_us, delay_us);
  std::mt19937 rng(seed);
  std::atomic<long> bad{0};
  std::atomic<int> running{0};
  for (int b = 0; b < bursts; b++) {
    const int n = 1 + (int)(rng() % (unsigned)max_n);
    std::unique_ptr<std::atomic<int>[]> cnt(new std::atomic<int>[n]);
    for (int i = 0; i < n; i++) cnt[i].store(0);
    const int tag = b;
    pool.parallel_for(n, [&, tag](int i) {
      running.fetch_add(1);
      if (i < 0 || i >= n || tag != b) bad.fetch_add(1);
      else cnt[i].fetch_add(1);
      if ((i & 7) == 0) std::this_thread::yield();
      running.fetch_sub(1);
    });
    if (running.load() != 0) bad.fetch_add(1);
    for (int i = 0; i < n; i++) bad.fetch_add(cnt[i].load() != 1);
  }
  return bad.load();
}

// The variable-base MSM (msm_var.hip) without a device: sum_i s_i P_i of n compressed points with window width c, from
// the kernels' recode and key function (vmsm.hpp), the buckets filled on the host from the (key, entry) pairs in the
// device's group layout, and the device path's host finish. Returns 0 with out32 set, -1 for bad arguments
// (n = 0 is the identity), or -4 (SPG_E_POINT) with *bad_index = the lowest index whose encoding does not decode.
int spgh_vmsm_emulate(const uint8_t* compressed, const uint64_t* scalars_mont, size_t n, int c, uint8_t* out32,
                      long* bad_index) {
  if (!out32 || c < kVmsmCMin || c > kVmsmCMax || (n && (!compressed || !scalars_mont))) return -1;
  if (n == 0) {
    memset(out32, 0, 32);
    return 0;
  }
  std::vector<Niels> pts(n);
  for (size_t i = 0; i < n; i++) {
    Ext P;
    if (!ext_decompress(compressed + 32 * i, P)) {
      if (bad_index) *bad_index = (long)i;
      return -4;
    }
    pts[i] = vmsm_niels_affine(P);
  }
  std::vector<Fq> s(n);
  for (size_t i = 0; i < n; i++) s[i] = ldq(scalars_mont + 4 * i);
  const size_t off = 0;
  vmsm_host(pts.data(), &off, &n, 1, s.data(), c, out32);
  return 0;
}
// the signed c-bit digits of one Montgomery scalar (vmsm_digit), 253 / c + 1 of them; returns their number
int spgh_vmsm_digits(const uint64_t* scalar_mont, int c, int* out) {
  if (c < kVmsmCMin || c > kVmsmCMax) return -1;
  const Fq k = fq_from_mont(ldq(scalar_mont));
  int carry = 0;
  const int W = vmsm_windows(c);
  for (int w = 0; w < W; w++) out[w] = vmsm_digit(k.l, c, w, carry);
  return W;
}

// spg_eqs_check's semantics on the host (eqcheck.hpp): the argument check the device entry makes before it launches
// anything (-1: malformed, as SPG_E_ARG), then every equation evaluated with hcurve.hpp. base: the nb base points as
// encodings (the device entry holds them resident). plan (optional): the term and sum kernels' grids for this call.
int spgh_eqs_check(const uint8_t* base, size_t nb, const uint8_t* compressed, size_t nc, const uint8_t* extended,
                   size_t ne, const uint8_t* forms, const uint32_t* operands, const uint64_t* scalars_mont,
                   const size_t* first, size_t E, uint8_t* sums, uint8_t* status, long* bad_term, unsigned* plan) {
  if (E && (!first || !status)) return -1;
  if (nb && !base) return -1;
  EqsView v;
  v.kinds = forms;
  v.refs = operands;
  v.scalars = (const Fq*)scalars_mont;
  v.first = first;
  v.E = E;
  v.compressed = compressed;
  v.nc = nc;
  v.extended = extended;
  v.ne = ne;
  v.nb = nb;
  if (eqs_validate(v)) return -1;
  if (plan) {
    const EqsPlan p = eqs_plan(v.T(), E);
    plan[0] = p.term_grid;
    plan[1] = p.sum_grid;
  }
  eqs_host_eval(v, base, sums, status, bad_term);
  return 0;
}

// the merge of the ranks' satisfiability reports behind spg_r1cs_sat_check and the check mode of a sharded
// spg_r1cs_prove (satcheck.hpp): reports = nranks spg_sat_report records, as the allgather delivers them
int spgh_sat_merge(const spg_sat_report* reports, int nranks, spg_sat_report* out) {
  if (!reports || !out || nranks < 1) return -1;
  sat_merge(reports, nranks, out);
  return 0;
}
// sat_descs / sat_decode (satcheck.hpp): the natural key of a packed table -> (p, q, row) and the stored (bit-reversed)
// position, out[0..4); -1 for a shape the entries refuse or a key past the domain
int spgh_sat_decode(const size_t* num_proofs, const size_t* num_cons, size_t P, uint64_t key, uint64_t* out) {
  std::vector<SatDesc> d;
  uint64_t total = 0;
  if (!P || sat_descs(num_proofs, num_cons, P, &d, &total) || key >= total) return -1;
  sat_decode(d, key, out, out + 1, out + 2, out + 3);
  return 0;
}

// merge_order (snark_shape.hpp), the section merge of SNARK::prove and SNARK::verify: sizes = the components'
// num_proofs lists back to back, lens[c] = the length of component c's list. Writes the component of every merged
// instance (at most sum(lens)) and returns their number, or -1 when the sizes give no order
long spgh_merge_order(const size_t* sizes, const size_t* lens, size_t ncomp, size_t* inst_map) {
  std::vector<std::vector<size_t>> comps(ncomp);
  std::vector<const std::vector<size_t>*> ptrs;
  for (size_t c = 0, o = 0; c < ncomp; o += lens[c++]) comps[c].assign(sizes + o, sizes + o + lens[c]);
  for (auto& c : comps) ptrs.push_back(&c);
  std::vector<size_t> map;
  if (!merge_order(ptrs, &map)) return -1;
  for (size_t i = 0; i < map.size(); i++) inst_map[i] = map[i];
  return (long)map.size();
}
// SnarkShape (snark_shape.hpp) of a program with Bb blocks. scalars = (num_inputs_unpadded, block_max_num_proofs,
// consis_num_proofs, total init phy / init vir / phy / vir accesses, mem_addr_ts_bits_size). head[14] = (P, bmax,
// consis, t_iphy, t_ivir, t_phy, t_vir, pairwise_size, perm_size, pw_nv, |pw_order|, pw_order padded to 3);
// per_block[7][Bb] = the first P entries of (order, bnp, bnp_pad, bnv, bphy, bvir, w2_size). Returns P
long spgh_snark_shape(size_t Bb, const size_t* nproofs, const size_t* nvars, const size_t* phy_ops, const size_t* vir_ops,
                      const size_t* scalars, size_t* head, size_t* per_block) {
  spg_snark_inputs a;
  memset(&a, 0, sizeof(a));
  a.block_num_instances_bound = Bb;
  a.num_inputs_unpadded = scalars[0];
  a.block_max_num_proofs = scalars[1];
  a.consis_num_proofs = scalars[2];
  a.total_num_init_phy_mem_accesses = scalars[3];
  a.total_num_init_vir_mem_accesses = scalars[4];
  a.total_num_phy_mem_accesses = scalars[5];
  a.total_num_vir_mem_accesses = scalars[6];
  a.mem_addr_ts_bits_size = scalars[7];
  const SnarkShape s(a, nproofs, nvars, phy_ops, vir_ops);
  const size_t h[11] = {s.P, s.bmax, s.consis, s.t_iphy, s.t_ivir, s.t_phy, s.t_vir, s.pairwise_size, s.perm_size,
                        s.pw_nv, s.pw_order.size()};
  memcpy(head, h, sizeof(h));
  for (size_t i = 0; i < 3; i++) head[11 + i] = i < s.pw_order.size() ? s.pw_order[i] : 0;
  const std::vector<size_t>* rows[6] = {&s.order, &s.bnp, &s.bnp_pad, &s.bnv, &s.bphy, &s.bvir};
  for (size_t p = 0; p < s.P; p++) {
    for (size_t k = 0; k < 6; k++) per_block[k * Bb + p] = (*rows[k])[p];
    per_block[6 * Bb + p] = s.w2_size(p);
  }
  return (long)s.P;
}
// block_width_violation (snark_shape.hpp), the check spg_snark_prove makes before any launch: the first executed
// block whose io / memory-operation part or whose matrix columns reach beyond its block_num_vars, or -1
long spgh_block_width_violation(size_t Bb, const size_t* nproofs, const size_t* nvars, const size_t* phy_ops,
                                const size_t* vir_ops, size_t niu, size_t stride, const spg_sparse_entry* const* entries,
                                const size_t* nnz) {
  if (!stride) return 0;
  const std::vector<size_t> need = block_cols_needed(Bb, stride, entries, nnz);
  return block_width_violation(Bb, nproofs, nvars, phy_ops, vir_ops, niu, stride, need.data());
}
// PePlan (pe_plan.hpp), the grouping and slab plan the spg_poly_eval_*_batched_* entries prove and verify by.
// instances = 0: the points form, n points of nv_list[0] scalars each in r_list (r_lens unused); else the instances
// form, polynomial i of nv_list[i] variables with a point of r_lens[i] scalars. Per term: term[6 i ..] = (group,
// coefficient exponent, bound, S, chunk, first slab); fitted (optional) receives its fitted point, nv_i scalars each,
// concatenated. Per group: grp[7 g ..] = (num_vars, Ls, Rs, first term, S, part_off, out_off). tot (optional) =
// (part_len, out_len, xblocks, proof list bytes). Returns the number of groups.
long spgh_pe_plan(int instances, size_t n, const size_t* nv_list, const uint64_t* r_list, const size_t* r_lens,
                  size_t* term, uint64_t* fitted, size_t* grp, size_t* tot) {
  size_t tot_r = 0;
  for (size_t i = 0; i < n; i++) tot_r += instances ? r_lens[i] : nv_list[0];
  std::vector<Fq> r(tot_r);
  for (size_t i = 0; i < tot_r; i++) r[i] = ldq(r_list + 4 * i);
  const PePlan p = instances ? pe_plan_instances(nv_list, r.data(), r_lens, n) : pe_plan_points(r.data(), n, nv_list[0]);
  size_t fo = 0;
  for (size_t i = 0; i < n; i++) {
    const PeTerm& t = p.terms[i];
    const size_t row[6] = {t.group, t.exp, t.bound ? (size_t)1 : 0, t.S, t.chunk, t.slab};
    memcpy(term + 6 * i, row, sizeof(row));
    for (size_t k = 0; fitted && k < t.r.size(); k++) stq(fitted + 4 * (fo + k), t.r[k]);
    fo += t.r.size();
  }
  for (size_t k = 0; k < p.groups.size(); k++) {
    const PeGroup& g = p.groups[k];
    const size_t row[7] = {g.nv, g.Ls, g.Rs, g.first, g.S, g.part_off, g.out_off};
    memcpy(grp + 7 * k, row, sizeof(row));
  }
  if (tot) {
    tot[0] = p.part_len, tot[1] = p.out_len, tot[2] = p.xblocks, tot[3] = pe_list_bytes(p);
  }
  return (long)p.groups.size();
}
// The disjoint-rounds walk (pe_walk_disjoint, pe_plan.hpp) the R1CS witness opening proves and verifies by: term i has
// the shape (num_proofs, num_inputs) = (shape[2 i], shape[2 i + 1]); group[i] and exp[i] receive its proof slot and
// coefficient exponent. Returns the number of groups.
long spgh_pe_walk_disjoint(size_t n, const size_t* shape, size_t* group, size_t* exp) {
  std::vector<std::pair<size_t, size_t>> s(n);
  for (size_t i = 0; i < n; i++) s[i] = {shape[2 * i], shape[2 * i + 1]};
  const PeWalk w = pe_walk_disjoint(s);
  std::copy(w.group.begin(), w.group.end(), group);
  std::copy(w.exp.begin(), w.exp.end(), exp);
  return (long)w.first.size();
}
// pe_plan_disjoint (pe_plan.hpp), the plan spg_pe_prove_disjoint proves by: term i has the shape (shape[2 i],
// shape[2 i + 1]) (powers of two, lg num_proofs <= rq_len), the point halves rq and ry. term, fitted, grp, tot: the row
// formats of spgh_pe_plan. Returns the number of groups.
long spgh_pe_plan_disjoint(size_t n, const size_t* shape, const uint64_t* rq, size_t rq_len, const uint64_t* ry,
                           size_t ry_len, size_t* term, uint64_t* fitted, size_t* grp, size_t* tot) {
  std::vector<size_t> np(n), ni(n);
  for (size_t i = 0; i < n; i++) np[i] = shape[2 * i], ni[i] = shape[2 * i + 1];
  std::vector<Fq> q(rq_len), y(ry_len);
  for (size_t i = 0; i < rq_len; i++) q[i] = ldq(rq + 4 * i);
  for (size_t i = 0; i < ry_len; i++) y[i] = ldq(ry + 4 * i);
  const PePlan p = pe_plan_disjoint(np.data(), ni.data(), n, q.data(), rq_len, y.data(), ry_len);
  size_t fo = 0;
  for (size_t i = 0; i < n; i++) {
    const PeTerm& t = p.terms[i];
    const size_t row[6] = {t.group, t.exp, t.bound ? (size_t)1 : 0, t.S, t.chunk, t.slab};
    memcpy(term + 6 * i, row, sizeof(row));
    for (size_t k = 0; fitted && k < t.r.size(); k++) stq(fitted + 4 * (fo + k), t.r[k]);
    fo += t.r.size();
  }
  for (size_t k = 0; k < p.groups.size(); k++) {
    const PeGroup& g = p.groups[k];
    const size_t row[7] = {g.nv, g.Ls, g.Rs, g.first, g.S, g.part_off, g.out_off};
    memcpy(grp + 7 * k, row, sizeof(row));
  }
  if (tot) {
    tot[0] = p.part_len, tot[1] = p.out_len, tot[2] = p.xblocks, tot[3] = pe_list_bytes(p);
  }
  return (long)p.groups.size();
}
// pe_plan_uni (pe_plan.hpp), the plan of spg_pe_prove_uni (per_term = 0: one output of R_size) and spg_pe_uni_evals
// (per_term = 1: one output per term). Per term: term[8 i ..] = (coefficient exponent, num_vars, Ls, Rs, S, chunk,
// part_off, out_off). tot = (part_len, out_len, xblocks, proof bytes, R_size). ends (optional, with r and c_base):
// the first and the last entry of every term's scaled table L'_i (pe_uni_scaled_Ls), 2 n scalars. Returns the number
// of terms.
long spgh_pe_plan_uni(int per_term, size_t n, const size_t* nv_list, size_t* term, size_t* tot, const uint64_t* r,
                      const uint64_t* c_base, uint64_t* ends) {
  const PeUniPlan p = pe_plan_uni(nv_list, n, per_term != 0);
  if (ends && r && c_base) {
    const std::vector<FqV> Lp = pe_uni_scaled_Ls(ldq(r), std::vector<size_t>(nv_list, nv_list + n), ldq(c_base));
    for (size_t i = 0; i < n; i++) stq(ends + 8 * i, Lp[i].front()), stq(ends + 8 * i + 4, Lp[i].back());
  }
  for (size_t i = 0; i < n; i++) {
    const PeUniTerm& t = p.terms[i];
    const size_t row[8] = {t.exp, t.nv, t.Ls, t.Rs, t.S, t.chunk, t.part_off, t.out_off};
    memcpy(term + 8 * i, row, sizeof(row));
  }
  tot[0] = p.part_len, tot[1] = p.out_len, tot[2] = p.xblocks, tot[3] = pe_proof_bytes(p.R_size), tot[4] = p.R_size;
  return (long)p.terms.size();
}

// ---- the launch shapes of msm_plan.hpp (tests/test_msm_plan_host.py; the GPU form tests choose their sizes by them).
// Knob values are arguments: the tests pass the table's defaults or the value a form sets.
int spgh_pick_window(size_t n_per_msm) { return pick_window(n_per_msm); }
int spgh_pick_small_window(size_t per, int forced) { return pick_small_window(per, forced); }
int spgh_msm_comb_rule(int has_idx, size_t B, size_t n, size_t tot) { return msm_comb_rule(has_idx != 0, B, n, tot); }
// out[12] = (c, NB, W, rows, m, S, log2m, seg_quad, quad, regroup, final_S, final_sl)
void spgh_msm_batch_route(size_t B, size_t per, int seg_m, int rows_cmax, int quad, long seg_quad_max, int final_sl,
                          int* out) {
  const MsmRoute r = msm_batch_route(B, per, seg_m, rows_cmax, quad != 0, seg_quad_max, final_sl);
  const int row[12] = {r.c, r.NB, r.W, r.rows, r.m, r.S, r.log2m, r.seg_quad, r.quad, r.regroup, r.final_S, r.final_sl};
  memcpy(out, row, sizeof(row));
}
// out[2] = (G, S)
void spgh_comb_rows_shape(size_t B, size_t per, size_t want, size_t gmax, size_t gmin, size_t* out) {
  comb_rows_shape(B, per, want, gmax, gmin, out, out + 1);
}
// out[2] = (G, spb)
void spgh_big_digit_blocks(int per, int spt, int* out) { big_digit_blocks(per, spt, out, out + 1); }
// out[3] = (G, BS, R) of bullet_comb_shape alone
void spgh_bullet_comb_shape(int P, int eg, int ebs, int er, int notree, int* out) {
  bullet_comb_shape(P, eg, ebs, er, notree, out, out + 1, out + 2);
}
// out[4] = (G, BS, R, wgs) of the launch over c-bit windows; returns 1 when it runs, 0 when the caller falls back
int spgh_bullet_comb_launch(int shape_P, int P, int c, int eg, int ebs, int er, int notree, int* out) {
  return bullet_comb_launch(shape_P, P, c, eg, ebs, er, notree, out, out + 1, out + 2, out + 3);
}
int spgh_bullet_parts_max() { return kBulletPartsMax; }
// out[2] = (K, BS)
void spgh_layer_grid(size_t W, size_t one_wg, size_t ept, unsigned* out) {
  int bs = 0;
  layer_grid(W, one_wg, ept, out, &bs);
  out[1] = (unsigned)bs;
}
int spgh_grid_for(uint32_t total, int cap) { return grid_for(total, cap); }

// The environment table (knobs.hpp) as text, one row per line: name, kind, default, lo, hi (the clamp; "-": none),
// live (0 / 1), description, tab separated. Writes at most cap bytes and returns the length of the whole text.
size_t spgh_knob_table(char* buf, size_t cap) {
  auto bound = [](long v) { return v == knob::kNoLo || v == knob::kNoHi ? std::string("-") : std::to_string(v); };
  std::string s;
  for (const knob::Row& r : knob::table())
    s += std::string(r.name) + "\t" + r.kind + "\t" + r.dflt + "\t" + bound(r.lo) + "\t" + bound(r.hi) + "\t" +
         (r.live ? "1" : "0") + "\t" + r.desc + "\n";
  if (cap) memcpy(buf, s.data(), std::min(cap, s.size()));
  return s.size();
}
// The workspace slot table (ws_slots.hpp) as text, one row per enumerator below kCount in order: ws_name, owner file,
// what it holds, tab separated. Writes at most cap bytes and returns the length of the whole text.
size_t spgh_ws_table(char* buf, size_t cap) {
  std::string s;
  for (size_t i = 0; i < (size_t)Ws::kCount; i++)
    s += std::string(ws_name((Ws)i)) + "\t" + ws_table()[i].owner + "\t" + ws_table()[i].what + "\n";
  if (cap) memcpy(buf, s.data(), std::min(cap, s.size()));
  return s.size();
}

// ---- spark_shape.hpp
// out[11] = (N, cells, nv_ops, nv_mem, nv_der, ops_len, mem_len, der_len, gens_n, ops_rows, mem_rows) of a batch of B
// matrices of 2^nvx x 2^nvy with at most max_nnz entries each
void spgh_spark_shape(size_t B, size_t max_nnz, size_t nvx, size_t nvy, size_t gens_nvx, size_t gens_nvy,
                      size_t gens_nnz, size_t gens_batch, size_t* out) {
  const size_t N = spark_num_ops(max_nnz), cells = spark_num_cells(nvx, nvy);
  const SparkShape sp(B, N, cells, gens_nvx, gens_nvy, gens_nnz, gens_batch);
  const size_t v[11] = {N,          cells,      sp.nv_ops,   sp.nv_mem,     sp.nv_der,    sp.ops_len,
                        sp.mem_len, sp.der_len, sp.gens_n(), sp.ops_rows(), sp.mem_rows()};
  memcpy(out, v, sizeof v);
}
// the refusals' messages ("" when accepted) into msg[cap]; return 1 when refused
static int refusal(const char* why, char* msg, size_t cap) {
  snprintf(msg, cap, "%s", why ? why : "");
  return why != nullptr;
}
int spgh_spark_commit_refusal(size_t B, size_t N, size_t cells, size_t nvx, size_t nvy, size_t gens_nvx,
                              size_t gens_nvy, size_t gens_nnz, size_t gens_batch, char* msg, size_t cap) {
  return refusal(spark_commit_refusal(B, N, cells, nvx, nvy, gens_nvx, gens_nvy, gens_nnz, gens_batch), msg, cap);
}
int spgh_spark_comm_refusal(size_t B, size_t N, size_t cells, size_t ops_rows, size_t mem_rows, size_t gens_nvx,
                            size_t gens_nvy, size_t gens_nnz, size_t gens_batch, char* msg, size_t cap) {
  return refusal(spark_comm_refusal(B, N, cells, ops_rows, mem_rows, gens_nvx, gens_nvy, gens_nnz, gens_batch), msg, cap);
}
// v[2W]: the W gathered entries first; filled with the levels above them. prod: the circuit's evaluate()
void spgh_tree_tops(uint64_t* v, size_t W, uint64_t* prod) {
  std::vector<Fq> t(2 * W, fq_zero());
  for (size_t i = 0; i < W; i++) t[i] = ldq(v + 4 * i);
  stq(prod, tree_tops_host(t.data(), W));
  for (size_t i = 0; i < 2 * W; i++) stq(v + 4 * i, t[i]);
}

// ---- r1cs_desc.hpp: the descriptor builders of the R1CS table kernels (tests/test_r1cs_tables_host.py)
// pqx_shape(rows, secs, cols): off[n] and the total
void spgh_pqx_shape(size_t n, const size_t* rows, size_t secs, const size_t* cols, size_t* off, size_t* total) {
  const PqxDev T = pqx_shape({rows, rows + n}, secs, {cols, cols + n}, npow2(n), 1, 1, 1);
  std::copy(T.off.begin(), T.off.end(), off);
  *total = T.total;
}
// k_spmv's list as the callers build it, over the instances [p0, p1) of P: the (proofs, 1, cons) table of those
// instances gives the offsets, then sp_descs. single: one matrix triple; log_ni = 1: the prover's form, 0: the
// multiply_vec_block seam's. out[8 p ..] = (dom_off, out_off, pi, lg_q, nrows, lg_rows, ni, lg_ni); returns p1 - p0
size_t spgh_r1cs_sp_descs(const size_t* proofs, const size_t* cons, const size_t* inputs, size_t p0, size_t p1, int single,
                          int log_ni, uint64_t* out) {
  const std::vector<size_t> lp(proofs + p0, proofs + p1), lc(cons + p0, cons + p1), li(inputs + p0, inputs + p1);
  const PqxDev Az = pqx_shape(lp, 1, lc, 1, 1, 1, 1);
  const std::vector<SpDesc> d = sp_descs(lp, lc, li, Az.off, p0, single != 0, log_ni != 0);
  for (size_t p = 0; p < d.size(); p++) {
    const uint64_t row[8] = {d[p].dom_off, d[p].out_off, d[p].pi, d[p].lg_q, d[p].nrows, d[p].lg_rows, d[p].ni, d[p].lg_ni};
    memcpy(out + 8 * p, row, sizeof(row));
  }
  return d.size();
}
// k_abc's list over the n matrices pi0, pi0 + 1, .. whose widths are inputs[pi0 ..]: the (1, secs, inputs) table gives
// the offsets, then abc_descs. out[6 p ..] = (dom_off, out_off, pi, ni, lg_ni, pad)
void spgh_r1cs_abc_descs(const size_t* inputs, size_t pi0, size_t n, size_t secs, uint64_t* out) {
  const std::vector<size_t> li(inputs + pi0, inputs + pi0 + n);
  const PqxDev ABC = pqx_shape(std::vector<size_t>(n, 1), secs, li, 1, 1, 1, 1);
  const std::vector<AbcDesc> d = abc_descs(ABC.ani, ABC.off, pi0);
  for (size_t p = 0; p < n; p++) {
    const uint64_t row[6] = {d[p].dom_off, d[p].out_off, d[p].pi, d[p].ni, d[p].lg_ni, d[p].pad};
    memcpy(out + 6 * p, row, sizeof(row));
  }
}
// mat_descs of a handle with Pm matrices: out[4 p ..] = (rp[0], rp[1], rp[2], cp)
void spgh_r1cs_mat_descs(size_t Pm, const uint64_t* rp_off, const uint64_t* cp_off, uint64_t* out) {
  spg_r1cs_inst I;
  I.num_instances = Pm;
  I.rp_off.assign(rp_off, rp_off + 3 * Pm);
  I.cp_off.assign(cp_off, cp_off + Pm);
  const std::vector<MatDesc> md = mat_descs(I);
  memcpy(out, md.data(), Pm * sizeof(MatDesc));
}

// ---- the multi-round decoders of hostmath.hpp. ev: a pair's 15 or a triple's 64 posted values; r: r_j (and r_j+1);
// out: (e0, e2, e3) of round j, then of round j + 1 (then of round j + 2)
void spgh_pair_rounds(const uint64_t* ev, const uint64_t* r, uint64_t* out) {
  Fq e[15], o[6];
  for (int i = 0; i < 15; i++) e[i] = ldq(ev + 4 * i);
  pair_round_j(e, o);
  pair_round_j1(e, ldq(r), o + 3);
  for (int i = 0; i < 6; i++) stq(out + 4 * i, o[i]);
}
void spgh_triple_rounds(const uint64_t* ev, const uint64_t* r, uint64_t* out) {
  Fq e[64], o[9], L[4], M[4];
  for (int i = 0; i < 64; i++) e[i] = ldq(ev + 4 * i);
  lagrange4(ldq(r), L);
  lagrange4(ldq(r + 4), M);
  triple_round_j(e, o);
  triple_round_j1(e, L, o + 3);
  triple_round_j2(e, L, M, o + 6);
  for (int i = 0; i < 9; i++) stq(out + 4 * i, o[i]);
}
// dims = 2: w[4] folded at r[2]; dims = 3: w[8] at r[3]
void spgh_fold_corners(int dims, const uint64_t* w, const uint64_t* r, uint64_t* out) {
  Fq c[8];
  for (int i = 0; i < (1 << dims); i++) c[i] = ldq(w + 4 * i);
  stq(out, dims == 2 ? fold_corners2(c, ldq(r), ldq(r + 4)) : fold_corners3(c, ldq(r), ldq(r + 4), ldq(r + 8)));
}

// The parse rule of one kind (knobs.hpp) on text (NULL: unset), with no environment involved. dflt[3], out[3]: the
// COSTS triple, else entry 0 alone (bools as 0 / 1, GB in bytes, STR: 1 when the text itself came back). Returns 0, or
// -1 for a kind the table does not know
int spgh_knob_parse(const char* kind, const char* text, const double* dflt, long lo, long hi, double* out) {
  const std::string k = kind;
  if (k == "ON") out[0] = knob::parse_on(text, dflt[0] != 0, lo, hi);
  else if (k == "OFF") out[0] = knob::parse_off(text, dflt[0] != 0, lo, hi);
  else if (k == "PRESENT") out[0] = knob::parse_present(text, dflt[0] != 0, lo, hi);
  else if (k == "INT") out[0] = knob::parse_int(text, (int)dflt[0], lo, hi);
  else if (k == "LONG") out[0] = (double)knob::parse_long(text, (long)dflt[0], lo, hi);
  else if (k == "GB") out[0] = (double)knob::parse_gb(text, dflt[0], lo, hi);
  else if (k == "STR") out[0] = text && knob::parse_str(text, nullptr, lo, hi) == text;
  else if (k == "COSTS") {
    const knob::StepCosts c = knob::parse_costs(text, knob::StepCosts{{(int)dflt[0], (int)dflt[1], (int)dflt[2]}}, lo, hi);
    for (int i = 0; i < 3; i++) out[i] = c.c[i];
  } else
    return -1;
  return 0;
}

}  // extern "C"

#ifdef SPGH_MAIN
// TSan driver (make sanitize -> lib/spg_pool_tsan): the pool stress test with its race-window delays, then the
// cross-rank exchange (comm.hpp) over an in-process allgather between threads, one thread per rank.
#include <stdio.h>

#include <condition_variable>
#include <mutex>
#include <thread>

namespace {
struct Barrier {
  std::mutex mu;
  std::condition_variable cv;
  int n, waiting = 0;
  unsigned gen = 0;
  explicit Barrier(int k) : n(k) {}
  void arrive_and_wait() {
    std::unique_lock<std::mutex> lk(mu);
    const unsigned g = gen;
    if (++waiting == n) {
      waiting = 0;
      gen++;
      cv.notify_all();
    } else {
      cv.wait(lk, [&] { return gen != g; });
    }
  }
};
struct ThreadComm {  // allgather between `n` threads through one shared buffer and a barrier per phase
  int n;
  std::vector<uint8_t> buf;
  Barrier bar;
  explicit ThreadComm(int nr) : n(nr), bar(nr) {}
};
struct RankUser {
  ThreadComm* c;
  int rank;
};
int thread_allgather(void* user, const void* send, size_t bytes, void* recv) {
  RankUser* u = (RankUser*)user;
  ThreadComm* c = u->c;
  if (u->rank == 0) c->buf.assign(bytes * c->n, 0);
  c->bar.arrive_and_wait();
  memcpy(c->buf.data() + bytes * u->rank, send, bytes);
  c->bar.arrive_and_wait();
  memcpy(recv, c->buf.data(), bytes * c->n);
  c->bar.arrive_and_wait();
  return 0;
}
}  // namespace

int main() {
  long bad = spgh_pool_stress(7, 300, 64, 0, 1) + spgh_pool_stress(7, 100, 16, 20, 2) + spgh_pool_stress(3, 200, 9, 5, 3);
  const int n = 4;
  ThreadComm comm(n);
  std::vector<std::thread> ts;
  std::vector<int> rcs(n), fails(n);
  std::vector<std::vector<uint64_t>> outs(n, std::vector<uint64_t>(12));
  for (int r = 0; r < n; r++)
    ts.emplace_back([&, r] {
      RankUser u{&comm, r};
      std::vector<uint64_t> mine(12);
      for (int i = 0; i < 12; i++) mine[i] = (uint64_t)(r + 1) * (i % 4 == 3 ? 1 : 1000003);
      rcs[r] = spgh_comm_sum(thread_allgather, &u, n, 0, mine.data(), 3, outs[r].data());
      std::vector<uint64_t> junk(12);
      fails[r] = spgh_comm_sum(thread_allgather, &u, n, r == 2 ? -3 : 0, mine.data(), 3, junk.data());
    });
  for (auto& t : ts) t.join();
  for (int r = 0; r < n; r++) {
    bad += rcs[r] != 0 || fails[r] != -3;
    bad += outs[r] != outs[0];
  }
  printf("pool stress + thread exchange: %ld violations\n", bad);
  return bad ? 1 : 0;
}
#endif
