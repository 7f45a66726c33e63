// spg — the R1CS handles of the C-ABI, made and freed: the generators (R1CSGens), the instance's matrices resident in
// HBM as CSR and merged CSC (r1cs_objs.hpp), and the witness sections, uploaded or assembled from resident parts.
#include "hostpoly.hpp"
#include "knobs.hpp"
#include "proto.hpp"
#include "r1cs_objs.hpp"

using namespace spg;

extern "C" int spg_r1cs_gens_new(spg_ctx* ctx, const uint8_t* label, size_t label_len, size_t num_vars,
                                 spg_r1cs_gens** out) {
  if (!ctx || !label || !out || num_vars == 0) return SPG_E_ARG;
  size_t nv = lg2(num_vars);
  size_t n_pc = (size_t)1 << (nv - nv / 2);  // poly_commit_gens_new: 2^right
  spg_r1cs_gens* rg = new spg_r1cs_gens();
  ProverGens& g = rg->g;
  size_t n = std::max<size_t>(n_pc + 1, 4);
  int rc = spg_gens_derive(ctx, label, label_len, n, &g.dev);
  if (rc) {
    delete rg;
    return rc;
  }
  g.host.init(g.dev->compressed, n + 1);
  g.n_pc = n_pc;
  g.gens_n.G.resize(n_pc);
  for (size_t i = 0; i < n_pc; i++) g.gens_n.G[i] = i;
  g.gens_n.h = n_pc + 1;
  g.gens_1.G = {n_pc};
  g.gens_1.h = n_pc + 1;
  g.gens_4.G = {0, 1, 2, 3};
  g.gens_4.h = 4;
  // warm the host fixed-base tables of the sigma-protocol generators
  for (size_t i : {(size_t)0, (size_t)1, (size_t)2, (size_t)3, (size_t)4, n_pc, n_pc + 1}) g.host.get(i);
  *out = rg;
  return SPG_OK;
}
extern "C" int spg_r1cs_gens_free(spg_ctx* ctx, spg_r1cs_gens* g) {
  if (!g) return SPG_OK;
  spg_gens_free(ctx, g->g.dev);
  delete g;
  return SPG_OK;
}
extern "C" int spg_r1cs_gens_download(spg_ctx* ctx, const spg_r1cs_gens* g, uint8_t* out, size_t* count) {
  if (!ctx || !g || !count) return SPG_E_ARG;
  *count = g->g.dev->n + 1;
  if (out) memcpy(out, g->g.dev->compressed, 32 * (g->g.dev->n + 1));
  return SPG_OK;
}

extern "C" int spg_r1cs_inst_new(spg_ctx* ctx, const spg_r1cs_instance* ci, spg_r1cs_inst** out) {
  if (!ctx || !ci || !out || !ci->num_instances || !ci->num_cons || !ci->nnz || !ci->entries) return SPG_E_ARG;
  if (!is_pow2(ci->max_num_cons) || !is_pow2(ci->num_vars))
    return set_err(ctx, SPG_E_ARG, "max_num_cons and num_vars must be powers of two");
  size_t Pm = ci->num_instances;
  std::vector<uint32_t> rowptr, col, colptr, crow;
  std::vector<Fq> val, cval;
  spg_r1cs_inst* I = new spg_r1cs_inst();
  I->num_instances = Pm;
  I->max_num_cons = ci->max_num_cons;
  I->num_vars = ci->num_vars;
  I->num_cons.assign(ci->num_cons, ci->num_cons + Pm);
  for (size_t p = 0; p < Pm; p++) {
    size_t nc = ci->num_cons[p];
    if (!is_pow2(nc) || nc > ci->max_num_cons) {
      delete I;
      return set_err(ctx, SPG_E_ARG, "num_cons must be powers of two <= max_num_cons");
    }
    // CSR per matrix (counting sort by row, stable in entry order)
    for (int m = 0; m < 3; m++) {
      size_t nnz = ci->nnz[3 * p + m];
      I->nnz.push_back(nnz);
      const spg_sparse_entry* E = ci->entries[3 * p + m];
      if (nnz && !E) {
        delete I;
        return SPG_E_ARG;
      }
      std::vector<uint32_t> cnt(nc + 1, 0);
      for (size_t e = 0; e < nnz; e++) {
        if (E[e].row >= nc || E[e].col >= ci->num_vars) {
          delete I;
          return set_err(ctx, SPG_E_ARG, "sparse entry out of range");
        }
        cnt[E[e].row + 1]++;
      }
      for (size_t r = 0; r < nc; r++) cnt[r + 1] += cnt[r];
      I->rp_off.push_back(rowptr.size());
      size_t base = col.size();
      for (size_t r = 0; r <= nc; r++) rowptr.push_back((uint32_t)(base + cnt[r]));
      col.resize(base + nnz);
      val.resize(base + nnz);
      std::vector<uint32_t> fill(cnt.begin(), cnt.end() - 1);
      for (size_t e = 0; e < nnz; e++) {
        size_t d = base + fill[E[e].row]++;
        col[d] = (uint32_t)E[e].col;
        val[d] = ld_fq(E[e].val);
      }
    }
    // merged CSC over A, B, C with tagged rows
    size_t ncol = ci->num_vars;
    std::vector<uint32_t> cnt(ncol + 1, 0);
    for (int m = 0; m < 3; m++)
      for (size_t e = 0; e < ci->nnz[3 * p + m]; e++) cnt[ci->entries[3 * p + m][e].col + 1]++;
    for (size_t c = 0; c < ncol; c++) cnt[c + 1] += cnt[c];
    I->cp_off.push_back(colptr.size());
    size_t base = crow.size();
    for (size_t c = 0; c <= ncol; c++) colptr.push_back((uint32_t)(base + cnt[c]));
    crow.resize(base + cnt[ncol]);
    cval.resize(base + cnt[ncol]);
    std::vector<uint32_t> fill(cnt.begin(), cnt.end() - 1);
    for (int m = 0; m < 3; m++)
      for (size_t e = 0; e < ci->nnz[3 * p + m]; e++) {
        const spg_sparse_entry& en = ci->entries[3 * p + m][e];
        size_t d = base + fill[en.col]++;
        crow[d] = (uint32_t)(en.row * 4 + m);
        cval[d] = ld_fq(en.val);
      }
  }
  if (col.size() >= 0xffffffffULL || crow.size() >= 0xffffffffULL || ci->max_num_cons >= (1ull << 30)) {
    delete I;
    return set_err(ctx, SPG_E_ARG, "instance too large");
  }
  auto up = [&](void** d, const void* h, size_t bytes) -> int {
    if (hipMalloc(d, bytes ? bytes : 16) != hipSuccess) return SPG_E_NOMEM;
    if (bytes && hipMemcpy(*d, h, bytes, hipMemcpyHostToDevice) != hipSuccess) return SPG_E_HIP;
    return 0;
  };
  int rc = up((void**)&I->d_rowptr, rowptr.data(), rowptr.size() * 4);
  if (!rc) rc = up((void**)&I->d_col, col.data(), col.size() * 4);
  if (!rc) rc = up((void**)&I->d_val, val.data(), val.size() * sizeof(Fq));
  if (!rc) rc = up((void**)&I->d_colptr, colptr.data(), colptr.size() * 4);
  if (!rc) rc = up((void**)&I->d_crow, crow.data(), crow.size() * 4);
  if (!rc) rc = up((void**)&I->d_cval, cval.data(), cval.size() * sizeof(Fq));
  if (rc) {
    spg_r1cs_inst_free(ctx, I);
    return set_err(ctx, rc, "instance upload");
  }
  *out = I;
  return SPG_OK;
}
extern "C" int spg_r1cs_inst_free(spg_ctx* ctx, spg_r1cs_inst* I) {
  (void)ctx;
  if (!I) return SPG_OK;
  hipFree(I->d_rowptr);
  hipFree(I->d_col);
  hipFree(I->d_val);
  hipFree(I->d_colptr);
  hipFree(I->d_crow);
  hipFree(I->d_cval);
  delete I;
  return SPG_OK;
}

static int witness_new(spg_ctx* ctx, const spg_witness_sec* secs, size_t nws, size_t p0, size_t p1,
                       spg_r1cs_witness** out) {
  if (!ctx || !secs || !out || nws == 0) return SPG_E_ARG;
  if (nws > 8) return set_err(ctx, SPG_E_ARG, "at most 8 witness sections (prefix_list)");
  spg_r1cs_witness* W = new spg_r1cs_witness();
  W->nws = nws;
  W->num_proofs.resize(nws);
  W->num_inputs.resize(nws);
  W->off.resize(nws);
  size_t total = 0;
  for (size_t w = 0; w < nws; w++) {
    const spg_witness_sec& s = secs[w];
    if (!s.num_instances || !s.num_proofs || !s.num_inputs || !s.w) {
      delete W;
      return SPG_E_ARG;
    }
    for (size_t p = 0; p < s.num_instances; p++) {
      if (!is_pow2(s.num_proofs[p]) || !is_pow2(s.num_inputs[p])) {
        delete W;
        return set_err(ctx, SPG_E_ARG, "witness section sizes must be powers of two");
      }
      W->num_proofs[w].push_back(s.num_proofs[p]);
      W->num_inputs[w].push_back(s.num_inputs[p]);
      bool here = s.num_instances == 1 || (p >= p0 && p < p1);
      if (here && !s.w[p]) {
        delete W;
        return set_err(ctx, SPG_E_ARG, "missing witness data for a resident instance");
      }
      W->off[w].push_back(here ? total : kNotResident);
      if (here) total += s.num_proofs[p] * s.num_inputs[p];
    }
  }
  W->total = total;
  if (!(W->d_w = (Fq*)dev_cache_get(ctx, total * sizeof(Fq) + 64))) {
    delete W;
    return set_err(ctx, SPG_E_NOMEM, "witness upload");
  }
  W->ptr.resize(nws);
  for (size_t w = 0; w < nws; w++)
    for (uint64_t o : W->off[w]) W->ptr[w].push_back(o == kNotResident ? nullptr : W->d_w + o);
  for (size_t w = 0; w < nws; w++)
    for (size_t p = 0; p < secs[w].num_instances; p++) {
      if (W->off[w][p] == kNotResident) continue;
      size_t n = W->num_proofs[w][p] * W->num_inputs[w][p];
      // Scalar([u64; 4]) and Fq(u32[8]) share the little-endian byte image. Streamed through the page-locked ring
      // (h2d_stream: host pool copies, DMA on the upload stream): the call returns once the caller's buffers are read,
      // with the last chunks' DMAs in flight and the context stream ordered after them (round 6; a pageable
      // hipMemcpyAsync ran at ~26 GB/s and was synchronised here)
      if (int rc = h2d_stream(ctx, W->d_w + W->off[w][p], secs[w].w[p], n * sizeof(Fq))) {
        spg_r1cs_witness_free(ctx, W);
        return rc;
      }
    }
  *out = W;
  return SPG_OK;
}
namespace spg {
// witness sections assembled from host or device parts (SNARK::prove's ProverWitnessSecInfo lists); an
// existing *inout whose total size matches is refilled in place
int witness_from_parts(spg_ctx* ctx, const std::vector<WPart>& secs, spg_r1cs_witness** inout) {
  if (secs.empty() || secs.size() > 8) return set_err(ctx, SPG_E_ARG, "1..8 witness sections");
  size_t total = 0;
  for (auto& w : secs) {
    if (w.num_proofs.empty() || w.num_proofs.size() != w.num_inputs.size() || w.src.size() != w.num_proofs.size())
      return set_err(ctx, SPG_E_ARG, "witness part shape");
    for (size_t p = 0; p < w.num_proofs.size(); p++) {
      if (!is_pow2(w.num_proofs[p]) || !is_pow2(w.num_inputs[p]))
        return set_err(ctx, SPG_E_ARG, "witness section sizes must be powers of two");
      total += w.num_proofs[p] * w.num_inputs[p];
    }
  }
  // parts already resident on this device (SNARK::prove's block_vars and exec buffers, alive and unchanged for
  // the whole prove) are read in place; only host parts are copied into d_w
  // (a buffer on another GPU is copied like a host part: k_spmv / k_z_fill would otherwise read it across devices)
  auto on_device = [ctx](const void* q) {
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, q) != hipSuccess) {
      (void)hipGetLastError();  // an unregistered host pointer: not an error of the prove
      return false;
    }
    return a.type == hipMemoryTypeDevice && a.device == ctx->device;
  };
  const bool in_place = knob::wit_in_place();
  std::vector<std::vector<char>> dev(secs.size());
  size_t host_total = 0;
  for (size_t w = 0; w < secs.size(); w++)
    for (size_t p = 0; p < secs[w].num_proofs.size(); p++) {
      const bool d = in_place && on_device(secs[w].src[p]);
      dev[w].push_back(d);
      if (!d) host_total += secs[w].num_proofs[p] * secs[w].num_inputs[p];
    }
  (void)total;
  spg_r1cs_witness* W = *inout;
  if (W && W->total < host_total) {
    spg_r1cs_witness_free(ctx, W);
    W = nullptr;
  }
  if (!W) {
    W = new spg_r1cs_witness();
    if (hipMalloc(&W->d_w, host_total * sizeof(Fq) + 64) != hipSuccess) {
      delete W;
      *inout = nullptr;
      return set_err(ctx, SPG_E_NOMEM, "witness");
    }
    W->total = host_total;
  }
  *inout = W;
  W->nws = secs.size();
  W->num_proofs.assign(secs.size(), {});
  W->num_inputs.assign(secs.size(), {});
  W->off.assign(secs.size(), {});
  W->ptr.assign(secs.size(), {});
  size_t o = 0;
  for (size_t w = 0; w < secs.size(); w++)
    for (size_t p = 0; p < secs[w].num_proofs.size(); p++) {
      size_t n = secs[w].num_proofs[p] * secs[w].num_inputs[p];
      W->num_proofs[w].push_back(secs[w].num_proofs[p]);
      W->num_inputs[w].push_back(secs[w].num_inputs[p]);
      if (dev[w][p]) {
        W->off[w].push_back(0);
        W->ptr[w].push_back(secs[w].src[p]);
        continue;
      }
      W->off[w].push_back(o);
      W->ptr[w].push_back(W->d_w + o);
      SPG_HIP(ctx, hipMemcpyAsync(W->d_w + o, secs[w].src[p], n * sizeof(Fq), hipMemcpyDefault, ctx->stream));
      o += n;
    }
  return 0;
}
}  // namespace spg

extern "C" int spg_r1cs_witness_new(spg_ctx* ctx, const spg_witness_sec* secs, size_t nws, spg_r1cs_witness** out) {
  return witness_new(ctx, secs, nws, 0, ~(size_t)0, out);
}
extern "C" int spg_r1cs_witness_new_shard(spg_ctx* ctx, const spg_witness_sec* secs, size_t nws, size_t p0,
                                          size_t p1, spg_r1cs_witness** out) {
  return witness_new(ctx, secs, nws, p0, p1, out);
}
extern "C" int spg_r1cs_witness_free(spg_ctx* ctx, spg_r1cs_witness* W) {
  if (!W) return SPG_OK;
  if (ctx) {
    h2d_sync(ctx);  // a streamed upload into it may still be in flight
    dev_cache_put(ctx, W->d_w, W->total * sizeof(Fq) + 64);  // kept for the next witness of this size
  } else {
    hipFree(W->d_w);
  }
  delete W;
  return SPG_OK;
}
