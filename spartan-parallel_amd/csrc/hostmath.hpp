// spg — host-only scalar helpers of the prover drivers (sizes, eq tables, round polynomials). No HIP: shared with
// the CPU test library (hostcheck.cpp), so the CPU suite checks these exact functions against the oracle and the
// reference's own known-answer tests (src/unipoly.rs:127-181, src/dense_mlpoly.rs:1234-1252).
#pragma once
#include <stddef.h>

#include <vector>

#include "host.hpp"

namespace spg {

inline size_t lg2(size_t x) {  // src/math.rs:14-21 (rounds up)
  size_t r = 0;
  while (((size_t)1 << r) < x) r++;
  return r;
}

inline size_t npow2(size_t x) {
  size_t r = 1;
  while (r < x) r <<= 1;
  return r;
}

// EqPolynomial::evals (src/dense_mlpoly.rs:76-92)
inline FqV eq_evals_host(const FqV& r) {
  FqV e((size_t)1 << r.size(), fq_one());
  size_t size = 1;
  for (size_t j = 0; j < r.size(); j++) {
    size *= 2;
    for (size_t i = size - 1;; i -= 2) {
      Fq s = e[i / 2];
      e[i] = fq_mul(s, r[j]);
      e[i - 1] = fq_sub(s, e[i]);
      if (i < 2) break;
    }
  }
  return e;
}

// DensePolynomial::new(z).evaluate(r) (src/dense_mlpoly.rs:361-367) for short host vectors
inline Fq dense_eval_host(FqV z, const FqV& r) {
  z.resize((size_t)1 << r.size(), fq_zero());
  FqV chi = eq_evals_host(r);
  Fq s = fq_zero();
  for (size_t i = 0; i < z.size(); i++) s = fq_add(s, fq_mul(z[i], chi[i]));
  return s;
}

// UniPoly::from_evals for degree 3 (src/unipoly.rs:23-54) and evaluate (:72-80)
inline FqV uni_from_evals3(const Fq e[4]) {
  static const Fq two_inv = fq_inv(fq_from_u64(2)), six_inv = fq_inv(fq_from_u64(6));
  Fq d = e[0];
  Fq three_e1 = fq_add(fq_add(e[1], e[1]), e[1]), three_e2 = fq_add(fq_add(e[2], e[2]), e[2]);
  Fq a = fq_mul(six_inv, fq_sub(fq_add(fq_sub(e[3], three_e2), three_e1), e[0]));
  Fq four_e2 = fq_dbl(fq_dbl(e[2]));
  Fq five_e1 = fq_add(fq_dbl(fq_dbl(e[1])), e[1]);
  Fq b = fq_mul(two_inv, fq_sub(fq_add(fq_sub(fq_dbl(e[0]), five_e1), four_e2), e[3]));
  Fq c = fq_sub(fq_sub(fq_sub(e[1], d), a), b);
  return {d, c, b, a};
}

inline Fq uni_eval(const FqV& c, const Fq& r) {
  Fq ev = c[0], pw = r;
  for (size_t i = 1; i < c.size(); i++) {
    ev = fq_add(ev, fq_mul(pw, c[i]));
    pw = fq_mul(pw, r);
  }
  return ev;
}

inline bool is_pow2(size_t x) { return x && !(x & (x - 1)); }

// ---- several cubic sumcheck rounds from the grid one launch posts (k_phase1_pair / k_phase2_pair, k_layer_pair,
// k_layer_triple): the round polynomials' (e0, e2, e3), each once the challenge before it is drawn, and the final
// claims from a vector's posted corners.

// the cubic Lagrange basis on the nodes 0..3 at r
inline void lagrange4(const Fq& r, Fq L[4]) {
  static const Fq inv2 = fq_inv(fq_from_u64(2)), inv6 = fq_inv(fq_from_u64(6));
  const Fq a0 = r, a1 = fq_sub(r, fq_one()), a2 = fq_sub(a1, fq_one()), a3 = fq_sub(a2, fq_one());
  const Fq a01 = fq_mul(a0, a1), a23 = fq_mul(a2, a3);
  L[0] = fq_neg(fq_mul(fq_mul(a1, a23), inv6));
  L[1] = fq_mul(fq_mul(a0, a23), inv2);
  L[2] = fq_neg(fq_mul(fq_mul(a01, a3), inv2));
  L[3] = fq_mul(fq_mul(a01, a2), inv6);
}
// A pair's 15 values of F(t, s), the round-j summand in its own and the next round's variable: ev[4 y + t] = F(t, Y)
// for t = 0..3 on the lines Y = 0, 2, 3 (y = 0, 1, 2), then ev[12 + x] = F(X, 1) at X = 0, 2, 3.
// Round j: F(X, 0) + F(X, 1) at X = 0, 2, 3
inline void pair_round_j(const Fq ev[15], Fq ej[3]) {
  ej[0] = fq_add(ev[0], ev[12]);
  ej[1] = fq_add(ev[2], ev[13]);
  ej[2] = fq_add(ev[3], ev[14]);
}
// round j + 1: the cubics t -> F(t, Y) at t = r_j
inline void pair_round_j1(const Fq ev[15], const Fq& r_j, Fq ej1[3]) {
  Fq L[4];
  lagrange4(r_j, L);
  for (int y = 0; y < 3; y++) {
    Fq acc = fq_zero();
    for (int k = 0; k < 4; k++) acc = fq_add(acc, fq_mul(L[k], ev[4 * y + k]));
    ej1[y] = acc;
  }
}
// A triple's 64 values F(t, s, u) = ev[t + 4 s + 16 u] on {0..3}^3. Round j: F(X, s, u) over s, u in {0, 1}
inline void triple_round_j(const Fq ev[64], Fq ej[3]) {
  for (int xi = 0; xi < 3; xi++) {
    const int X = xi == 0 ? 0 : xi + 1;
    ej[xi] = fq_add(fq_add(ev[X], ev[X + 4]), fq_add(ev[X + 16], ev[X + 20]));
  }
}
// round j + 1: t -> F(t, Y, 0) + F(t, Y, 1) at t = r_j, Y = 0, 2, 3 (L = lagrange4(r_j))
inline void triple_round_j1(const Fq ev[64], const Fq L[4], Fq ej1[3]) {
  for (int yi = 0; yi < 3; yi++) {
    const int Y = yi == 0 ? 0 : yi + 1;
    Fq acc = fq_zero();
    for (int a = 0; a < 4; a++) acc = fq_add(acc, fq_mul(L[a], fq_add(ev[a + 4 * Y], ev[a + 4 * Y + 16])));
    ej1[yi] = acc;
  }
}
// round j + 2: (t, s) -> F(t, s, Z) at (r_j, r_j+1), Z = 0, 2, 3 (L = lagrange4(r_j), M = lagrange4(r_j+1))
inline void triple_round_j2(const Fq ev[64], const Fq L[4], const Fq M[4], Fq ej2[3]) {
  for (int zi = 0; zi < 3; zi++) {
    const int Z = zi == 0 ? 0 : zi + 1;
    Fq acc = fq_zero();
    for (int b = 0; b < 4; b++) {
      Fq row = fq_zero();
      for (int a = 0; a < 4; a++) row = fq_add(row, fq_mul(L[a], ev[a + 4 * b + 16 * Z]));
      acc = fq_add(acc, fq_mul(M[b], row));
    }
    ej2[zi] = acc;
  }
}
// a vector's 2 x 2 corners w[2 t + s] (p00, p01, p10, p11) folded at (r_j, r_j+1): bound_poly_var_top twice
inline Fq fold_corners2(const Fq w[4], const Fq& rj, const Fq& rj1) {
  const Fq q0 = fq_add(w[0], fq_mul(rj, fq_sub(w[2], w[0]))), q1 = fq_add(w[1], fq_mul(rj, fq_sub(w[3], w[1])));
  return fq_add(q0, fq_mul(rj1, fq_sub(q1, q0)));
}
// its 2 x 2 x 2 corners w[4 t + 2 s + u] folded at (r_j, r_j+1, r_j+2)
inline Fq fold_corners3(const Fq w[8], const Fq& rj, const Fq& rj1, const Fq& rj2) {
  Fq q[4];
  for (int j = 0; j < 4; j++) q[j] = fq_add(w[j], fq_mul(rj, fq_sub(w[j + 4], w[j])));
  const Fq y0 = fq_add(q[0], fq_mul(rj1, fq_sub(q[2], q[0]))), y1 = fq_add(q[1], fq_mul(rj1, fq_sub(q[3], q[1])));
  return fq_add(y0, fq_mul(rj2, fq_sub(y1, y0)));
}

}  // namespace spg
