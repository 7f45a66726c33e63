// spg — device twin of csrc/hostcheck.cpp (lib/libspg_devcheck.so, test infrastructure only): the product's
// field / curve / quad / recode / block-sum headers, unchanged, each primitive behind a trivial kernel, so
// tests/test_gpu_primitives.py can feed the device forms (the v_mad_u64_u32 column accumulator, __builtin_addc,
// the Fermat inverse, the DPP quad arithmetic) the edge operands that whole MSMs and proofs reach with
// probability ~2^-32. Straight-line code and __syncthreads only: no mailbox, ticket or spin-wait helper is
// wrapped. Op codes are those of spgh_fq_op / spgh_fp_op / spgh_point_op, so one driver feeds both libraries.
// Every entry allocates, copies in, launches once, copies out, and returns the HIP error code (0 = ok).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../spartan-parallel_amd/csrc/bullet.hpp"
#include "../../spartan-parallel_amd/csrc/cube.hpp"
#include "../../spartan-parallel_amd/csrc/curve.hpp"
#include "../../spartan-parallel_amd/csrc/field.hpp"
#include "../../spartan-parallel_amd/csrc/qsum.hpp"
#include "../../spartan-parallel_amd/csrc/quad.hpp"

using namespace spg;

namespace {

// device buffers of one call: freed together, the first HIP error kept
struct Bufs {
  std::vector<void*> p;
  hipError_t err = hipSuccess;
  void note(hipError_t e) {
    if (err == hipSuccess && e != hipSuccess) err = e;
  }
  void* in(const void* h, size_t bytes) {  // null host pointer: no buffer
    if (!h || err != hipSuccess) return nullptr;
    void* d = nullptr;
    note(hipMalloc(&d, bytes ? bytes : 1));
    if (d) p.push_back(d);
    if (d && bytes) note(hipMemcpy(d, h, bytes, hipMemcpyHostToDevice));
    return d;
  }
  void* out(size_t bytes) {
    if (err != hipSuccess) return nullptr;
    void* d = nullptr;
    note(hipMalloc(&d, bytes ? bytes : 1));
    if (d) p.push_back(d);
    if (d && bytes) note(hipMemset(d, 0, bytes));
    return d;
  }
  // after the launch: launch error, synchronisation result, then the copy back
  int finish(void* h, const void* d, size_t bytes) {
    note(hipGetLastError());
    note(hipDeviceSynchronize());
    if (err == hipSuccess && bytes) note(hipMemcpy(h, d, bytes, hipMemcpyDeviceToHost));
    return done();
  }
  int done() {
    for (void* d : p) (void)hipFree(d);
    p.clear();
    return (int)err;
  }
};

constexpr int kBS = 256;
inline unsigned blocks(size_t n, int per = kBS) { return (unsigned)((n + per - 1) / per); }

__device__ __forceinline__ Fq ldq(const Fq* p, size_t i) { return p ? p[i] : fq_zero(); }

// ---------------------------------------------------------------- Fq, one thread per element
__global__ void __launch_bounds__(kBS) k_fq_op(int op, const Fq* __restrict__ a, const Fq* __restrict__ b,
                                               Fq* __restrict__ out, size_t n) {
  const size_t i = (size_t)blockIdx.x * kBS + threadIdx.x;
  if (i >= n) return;
  const Fq x = a[i], y = ldq(b, i);
  Fq r;
  switch (op) {
    case 0: r = fq_add(x, y); break;
    case 1: r = fq_sub(x, y); break;
    case 2: r = fq_mul(x, y); break;
    case 3: r = fq_neg(x); break;
    case 4: r = fq_sqr(x); break;
    case 5: r = fq_inv(x); break;
    case 6: r = fq_from_mont(x); break;
    case 8: r = fq_mul_ps(x, y); break;
    case 9: r = fq_mul32(x, y); break;
    default: r = fq_to_mont(x); break;
  }
  out[i] = r;
}

// ---------------------------------------------------------------- Fp, one thread per element
__global__ void __launch_bounds__(kBS) k_fp_op(int op, const Fp* __restrict__ a, const Fp* __restrict__ b,
                                               Fp* __restrict__ out, size_t n) {
  const size_t i = (size_t)blockIdx.x * kBS + threadIdx.x;
  if (i >= n) return;
  const Fp x = a[i], y = b ? b[i] : fp_zero();
  Fp r;
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
  out[i] = r;
}

// ---------------------------------------------------------------- curve, one thread per point
// a point operand: a 32-byte encoding (ext_decompress) or a raw 128-byte extended point (X, Y, Z, T limbs as given)
__device__ __forceinline__ bool load_point(const uint8_t* __restrict__ src, size_t i, int raw, Ext& P) {
  if (raw) {
    P = reinterpret_cast<const Ext*>(src)[i];
    return true;
  }
  return ext_decompress(src + 32 * i, P);
}

__global__ void __launch_bounds__(64) k_point_op(int op, const uint8_t* __restrict__ a, const uint8_t* __restrict__ b,
                                                 uint8_t* __restrict__ out, int32_t* __restrict__ ok, size_t n,
                                                 int raw) {
  const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  Ext P, Q, R;
  if (op == 6) {
    ext_compress(ristretto_from_uniform_bytes(a + 64 * i), out + 32 * i);
    ok[i] = 1;
    return;
  }
  bool good = load_point(a, i, raw, P);
  if (op == 0 || op == 2 || op == 3) good = load_point(b, i, raw, Q) && good;
  if (!good) {
    ok[i] = 0;
    return;
  }
  switch (op) {
    case 0: R = ext_add(P, Q); break;
    case 1: R = ext_dbl(P); break;
    case 2: R = ext_madd(P, ext_to_niels(Q), false); break;
    case 3: R = ext_madd(P, ext_to_niels(Q), true); break;
    case 4: R = niels_to_ext(ext_to_niels(P)); break;
    default: R = P; break;  // 5: decompress (or a raw point) -> compress
  }
  ext_compress(R, out + 32 * i);
  ok[i] = 1;
}

// ---------------------------------------------------------------- quads, four lanes per point
__global__ void __launch_bounds__(kBS) k_to_niels(const Ext* __restrict__ Q, Niels* __restrict__ tab, int n) {
  const int i = blockIdx.x * kBS + threadIdx.x;
  if (i < n) tab[i] = ext_to_niels(Q[i]);
}

// op: 0 quad_add, 1 quad_dbl, 2 / 3 quad_madd + / - (niels_coord from tab), 4 quad_add_op with the second operand
// handed over in LDS by the mirrored quad of the workgroup (slot S - 1 - slot; a switched-off quad hands over the
// identity), 5 quad_put (every lane reads the whole slot back). Every lane encodes its own copy of the result.
template <int BS>
__global__ void __launch_bounds__(BS) k_quad_op(int op, const Ext* __restrict__ A, const Ext* __restrict__ B,
                                                const Niels* __restrict__ tab, uint8_t* __restrict__ out, int P) {
  constexpr int S = BS / 4;
  __shared__ uint32_t pts[soa_words<Ext, S>()];
  const int t = threadIdx.x, q = t & 3, slot = t >> 2;
  const int p = blockIdx.x * S + slot;
  Ext acc = ext_identity(), other = ext_identity();
  if (p < P) {
    acc = A[p];
    if (op == 0) {
      acc = quad_add(acc, B[p], q);
    } else if (op == 1) {
      acc = quad_dbl(acc, q);
    } else if (op == 2 || op == 3) {
      bool neg;
      const Fp qv = niels_coord(tab, (uint32_t)p | (op == 3 ? 0x80000000u : 0u), q, &neg);
      acc = quad_madd(acc, qv, neg, q);
    } else if (op == 4) {
      other = B[p];
    }
  }
  if (op == 4) {
    quad_put_op<S>(pts, slot, other, q);
    __syncthreads();
    acc = quad_add_op(acc, quad_get_op<S>(pts, S - 1 - slot, q), q);
  } else if (op == 5) {
    quad_put<S>(pts, slot, acc, q);
    __syncthreads();
    Fp c[4];
    for (int k = 0; k < 4; k++)
      for (int i = 0; i < 8; i++) c[k].l[i] = pts[(k * 8 + i) * S + slot];
    acc.X = c[0]; acc.Y = c[1]; acc.Z = c[2]; acc.T = c[3];
  }
  if (p < P) ext_compress(acc, out + 32 * ((size_t)p * 4 + q));
}

// ---------------------------------------------------------------- signed-window recode
// thread (i, jg): the entries of window group jg of scalar i, as k_bullet_comb / k_comb_msm_parts call it
template <int C, int G>
__global__ void __launch_bounds__(kBS) k_recode(const Fq* __restrict__ k, const uint32_t* __restrict__ slot, int NS,
                                                uint32_t* __restrict__ out, int n) {
  constexpr int W = 253 / C + 1, WG = (W + G - 1) / G;
  const int g = blockIdx.x * kBS + threadIdx.x;
  const int i = g / G, jg = g - i * G;
  if (i >= n) return;
  uint32_t ent[WG];
  comb_window_entries<C, WG>(k[i], jg * WG, (int)slot[i], NS, ent);
#pragma unroll
  for (int x = 0; x < WG; x++) out[((size_t)i * G + jg) * WG + x] = ent[x];
}

// ---------------------------------------------------------------- block sums and lane-argument helpers
template <int BS>
__global__ void __launch_bounds__(BS) k_quad_block_sum(const Fq* __restrict__ in, Fq* __restrict__ out) {
  Fq e = in[(size_t)blockIdx.x * BS + threadIdx.x];
  quad_block_sum<BS>(e);
  if (threadIdx.x < 3) out[3 * blockIdx.x + threadIdx.x] = e;
}
template <int BS>
__global__ void __launch_bounds__(BS) k_row_block_sum(const Fq* __restrict__ in, Fq* __restrict__ out) {
  Fq e = in[(size_t)blockIdx.x * BS + threadIdx.x];
  row_block_sum<BS>(e);
  if (threadIdx.x < 16) out[16 * blockIdx.x + threadIdx.x] = e;
}
// op: 2 line_at(a, b, arg), 3 fq_small(a, arg), 4 cube_at(a, b, c, d, arg >> 2, arg & 3)
__global__ void __launch_bounds__(kBS) k_lane_op(int op, const Fq* __restrict__ a, const Fq* __restrict__ b,
                                                 const Fq* __restrict__ c, const Fq* __restrict__ d,
                                                 const int32_t* __restrict__ arg, Fq* __restrict__ out, size_t n) {
  const size_t i = (size_t)blockIdx.x * kBS + threadIdx.x;
  if (i >= n) return;
  const int g = arg[i];
  Fq r;
  if (op == 2) r = line_at(a[i], ldq(b, i), g);
  else if (op == 3) r = fq_small(a[i], g);
  else r = cube_at(a[i], ldq(b, i), ldq(c, i), ldq(d, i), g >> 2, g & 3);
  out[i] = r;
}

}  // namespace

extern "C" {

// op: 0 add, 1 sub, 2 mul, 3 neg, 4 square, 5 invert (Fermat chain), 6 from_mont, 7 to_mont, 8 mul_ps, 9 mul32
int spgd_fq_op(int op, const uint64_t* a, const uint64_t* b, uint64_t* out, size_t n) {
  Bufs B;
  const Fq* da = (const Fq*)B.in(a, 32 * n);
  const Fq* db = (const Fq*)B.in(b, 32 * n);
  Fq* dout = (Fq*)B.out(32 * n);
  if (B.err != hipSuccess || !n) return B.done();
  hipLaunchKernelGGL(k_fq_op, dim3(blocks(n)), dim3(kBS), 0, 0, op, da, db, dout, n);
  return B.finish(out, dout, 32 * n);
}

// op codes of spgh_fp_op (0 .. 12; 8 .. 11 raw, the others canonicalised); 8 x u32 per element, loose allowed
int spgd_fp_op(int op, const uint32_t* a, const uint32_t* b, uint32_t* out, size_t n) {
  Bufs B;
  const Fp* da = (const Fp*)B.in(a, 32 * n);
  const Fp* db = (const Fp*)B.in(b, 32 * n);
  Fp* dout = (Fp*)B.out(32 * n);
  if (B.err != hipSuccess || !n) return B.done();
  hipLaunchKernelGGL(k_fp_op, dim3(blocks(n)), dim3(kBS), 0, 0, op, da, db, dout, n);
  return B.finish(out, dout, 32 * n);
}

// op: 0 add, 1 double, 2 madd via niels, 3 madd negated (as spgh_point_op), 4 ext_to_niels -> niels_to_ext,
// 5 decompress -> compress, 6 ristretto_from_uniform_bytes (a: 64 bytes per element). raw = 0: a, b are 32-byte
// encodings; raw = 1: 128-byte extended points (X, Y, Z, T, 8 x u32 each, used as given). out: n encodings;
// ok[i] = 0 where an operand did not decode (out[i] left zero).
int spgd_point_op(int op, const uint8_t* a, const uint8_t* b, uint8_t* out, int32_t* ok, size_t n, int raw) {
  Bufs B;
  const size_t el = op == 6 ? 64 : (raw ? 128 : 32);
  const uint8_t* da = (const uint8_t*)B.in(a, el * n);
  const uint8_t* db = (const uint8_t*)B.in(b, el * n);
  uint8_t* dout = (uint8_t*)B.out(32 * n + 4 * n);
  if (B.err != hipSuccess || !n) return B.done();
  if ((op == 0 || op == 2 || op == 3) && !db) return B.done(), (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(k_point_op, dim3(blocks(n, 64)), dim3(64), 0, 0, op, da, db, dout, (int32_t*)(dout + 32 * n), n,
                     raw);
  std::vector<uint8_t> h(36 * n);
  const int rc = B.finish(h.data(), dout, 36 * n);
  if (rc == 0) {
    memcpy(out, h.data(), 32 * n);
    memcpy(ok, h.data() + 32 * n, 4 * n);
  }
  return rc;
}

// op: 0 quad_add, 1 quad_dbl, 2 / 3 quad_madd + / -, 4 quad_add_op (operand of B[mirror quad] through LDS),
// 5 quad_put; a, b: n raw 128-byte extended points; out: 4 n encodings, lane q of quad p at 4 p + q;
// bs: workgroup size, 64 or 256
int spgd_quad_op(int op, const uint32_t* a, const uint32_t* b, uint8_t* out, size_t n, int bs) {
  if (bs != 64 && bs != 256) return (int)hipErrorInvalidValue;
  Bufs B;
  const Ext* da = (const Ext*)B.in(a, 128 * n);
  const Ext* db = (const Ext*)B.in(b, 128 * n);
  Niels* tab = (Niels*)B.out(sizeof(Niels) * n);
  uint8_t* dout = (uint8_t*)B.out(128 * n);
  if (B.err != hipSuccess || !n) return B.done();
  if ((op == 0 || op == 2 || op == 3 || op == 4) && !db) return B.done(), (int)hipErrorInvalidValue;
  if (op == 2 || op == 3) hipLaunchKernelGGL(k_to_niels, dim3(blocks(n)), dim3(kBS), 0, 0, db, tab, (int)n);
  const unsigned nb = blocks(4 * n, bs);
  if (bs == 64)
    hipLaunchKernelGGL(k_quad_op<64>, dim3(nb), dim3(64), 0, 0, op, da, db, tab, dout, (int)n);
  else
    hipLaunchKernelGGL(k_quad_op<256>, dim3(nb), dim3(256), 0, 0, op, da, db, tab, dout, (int)n);
  return B.finish(out, dout, 128 * n);
}

// comb_window_entries<C, WG> with WG = ceil(W / G), W = 253 / C + 1, for the (C, G) of msm.hip's launch tables
// (bullet_round_comb / comb_msm_parts): (13, 4), (13, 10), (12, 4), (12, 8), (12, 11). k: n canonical scalars
// (8 x u32), slot: n generator slots; out: n x (G WG) entries, window w at index w (those past W - 1 stay all ones).
int spgd_recode(int C, int G, const uint32_t* k, const uint32_t* slot, int NS, uint32_t* out, size_t n) {
  const int W = 253 / C + 1, WG = (W + G - 1) / G;
  Bufs B;
  const Fq* dk = (const Fq*)B.in(k, 32 * n);
  const uint32_t* ds = (const uint32_t*)B.in(slot, 4 * n);
  const size_t ob = 4 * n * G * WG;
  uint32_t* dout = (uint32_t*)B.out(ob);
  if (B.err != hipSuccess || !n) return B.done();
  const dim3 grid(blocks(n * G)), blk(kBS);
#define SPGD_RC(CC, GG) hipLaunchKernelGGL((k_recode<CC, GG>), grid, blk, 0, 0, dk, ds, NS, dout, (int)n)
  if (C == 13 && G == 4) SPGD_RC(13, 4);
  else if (C == 13 && G == 10) SPGD_RC(13, 10);
  else if (C == 12 && G == 4) SPGD_RC(12, 4);
  else if (C == 12 && G == 8) SPGD_RC(12, 8);
  else if (C == 12 && G == 11) SPGD_RC(12, 11);
  else return B.done(), (int)hipErrorInvalidValue;
#undef SPGD_RC
  return B.finish(out, dout, ob);
}

// op 0: quad_block_sum<bs>, op 1: row_block_sum<bs> over n / bs workgroups of bs threads (bs 64 or 256, the sizes
// layer.hpp, sumcheck.hip and spark.hip launch them with); thread t's value is a[blk bs + t]; out: 3 (op 0) or
// 16 (op 1) sums per workgroup. op 2: line_at(a, b, arg), 3: fq_small(a, arg), 4: cube_at(a, b, c, d, arg >> 2,
// arg & 3), one thread per element.
int spgd_block_sum(int op, int bs, const uint64_t* a, const uint64_t* b, const uint64_t* c, const uint64_t* d,
                   const int32_t* arg, uint64_t* out, size_t n) {
  Bufs B;
  const Fq* da = (const Fq*)B.in(a, 32 * n);
  if (B.err != hipSuccess || !n || !da) return B.done();
  if (op == 0 || op == 1) {
    if ((bs != 64 && bs != 256) || n % bs) return B.done(), (int)hipErrorInvalidValue;
    const unsigned nb = (unsigned)(n / bs);
    const size_t ob = 32 * (size_t)nb * (op == 0 ? 3 : 16);
    Fq* dout = (Fq*)B.out(ob);
    if (B.err != hipSuccess) return B.done();
    if (op == 0 && bs == 64) hipLaunchKernelGGL(k_quad_block_sum<64>, dim3(nb), dim3(64), 0, 0, da, dout);
    else if (op == 0) hipLaunchKernelGGL(k_quad_block_sum<256>, dim3(nb), dim3(256), 0, 0, da, dout);
    else if (bs == 64) hipLaunchKernelGGL(k_row_block_sum<64>, dim3(nb), dim3(64), 0, 0, da, dout);
    else hipLaunchKernelGGL(k_row_block_sum<256>, dim3(nb), dim3(256), 0, 0, da, dout);
    return B.finish(out, dout, ob);
  }
  const Fq* db = (const Fq*)B.in(b, 32 * n);
  const Fq* dc = (const Fq*)B.in(c, 32 * n);
  const Fq* dd = (const Fq*)B.in(d, 32 * n);
  const int32_t* dg = (const int32_t*)B.in(arg, 4 * n);
  Fq* dout = (Fq*)B.out(32 * n);
  if (B.err != hipSuccess) return B.done();
  if (!dg || op < 2 || op > 4) return B.done(), (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(k_lane_op, dim3(blocks(n)), dim3(kBS), 0, 0, op, da, db, dc, dd, dg, dout, n);
  return B.finish(out, dout, 32 * n);
}

}  // extern "C"
