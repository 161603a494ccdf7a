// groth16_batch.hip -- many Groth16 proofs of ONE circuit in one call (kg_groth16_prove_batch): one CRS, `count` witnesses.
//
// A short proof is bound by launches and host chains, not by arithmetic (groth16.hip: ~35 launches, five 255-step host finishes and four
// blinding chains per proof).  Here a launch group of proofs shares every launch: one fill kernel pads the evaluation vectors and builds
// z = x || w, the batched transform (ntt_batch.hip) runs idft and coset_dft over all 3 g rows and coset_idft over the g rows of h, the
// point-wise step runs over the g n contiguous elements, five batched short MSMs (msm_small_batch.hip) leave the sums on the device, and
// three kernels assemble the proofs (groth16_assemble.h): the G1 chains with one lane per (proof, chain), the G2 chain and B with one lane
// per proof, and a finishing lane per proof for A and C.  Everything is enqueued on the context's stream; nothing crosses to the host and
// no worker thread is involved.  The number of launches does not depend on the group's size.
// kg_groth16_prove_r1cs_batch is the same from the witnesses alone: the constraint matrices take the place of the evaluation vectors, the
// fill kernel zeroes the rows and three batched CSR products (vec.hip: r1cs_prod_enqueue) write A z, B z, C z straight into them.
#include "common.h"
#include "groth16_qap.h"
#include "groth16_batch.h"
#include "r1cs_batch.h"
#include "groth16_assemble.h"
#include "chain_lds.h"
#include <climits>

using namespace kg;

namespace {

// ---- fill: padded rows and z ------------------------------------------------------------------------------------------------------------
struct G16FillArgs {
  const uint64_t* src[3];                                // the three evaluation arrays, at the group's first proof (null in the R1CS form)
  const uint64_t *x, *w;
  size_t eval_stride, x_stride, w_stride, m, l, nz, n, g;
  uint64_t* dst;                                         // [3][g][n] then [g][nz]
};
// element e of the group's polynomial and z arrays <- the caller's strided arrays (zero beyond m); one 32-byte element per lane.
// EVALS = false (the R1CS form): there are no evaluation arrays, the rows are zeroed whole -- the batched products fill [0, m) next
template <bool EVALS>
__global__ void __launch_bounds__(256) k_g16_fill(G16FillArgs a) {
  KG_SERVICE_PRIO();
  const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t rows = 3 * a.g * a.n;
  if (e >= rows + a.g * a.nz) return;
  uint32_t v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (e < rows) {
    if constexpr (EVALS) {
      const size_t row = e / a.n, i = e - row * a.n, vec = row / a.g, b = row - vec * a.g;
      const uint64_t* s = vec == 0 ? a.src[0] : (vec == 1 ? a.src[1] : a.src[2]);
      if (i < a.m) load_words(s, b * a.eval_stride + i, v);
    }
  } else {
    const size_t t = e - rows, b = t / a.nz, j = t - b * a.nz;
    if (j < a.l) load_words(a.x, b * a.x_stride + j, v);
    else load_words(a.w, b * a.w_stride + (j - a.l), v);
  }
  store_words(a.dst, e, v);
}

// ---- the assembly ------------------------------------------------------------------------------------------------------------------------
// (the LDS operand columns, the point loaders and the affine writer: chain_lds.h, shared with points_fold.hip)
struct G16VkG1 { uint32_t alpha[16], beta1[16], delta1[16]; };       // affine x | y, ABI words
struct G16VkG2 { uint32_t beta2[32], delta2[32]; };

// Lane t = 4 * proof + role runs chain `role` (0 .. 3) of its proof; the result goes to column t of `chains` (raw limbs, structure of
// arrays over the 4 g lanes).  The lanes differ in data only: every lane reads its proof's two sums and picks its operands word by word.
__global__ void __launch_bounds__(G16_NT) k_g16_chains_g1(G16VkG1 vk, const uint64_t* __restrict__ d_r, const uint64_t* __restrict__ d_s,
                                                          const uint64_t* __restrict__ sa, const uint8_t* __restrict__ sa_inf,
                                                          const uint64_t* __restrict__ sb1, const uint8_t* __restrict__ sb1_inf, size_t g,
                                                          uint32_t* __restrict__ chains) {
  __shared__ uint32_t lds[3 * PointIO<Fq>::NW * G16_NT];
  const size_t t = (size_t)blockIdx.x * G16_NT + threadIdx.x;
  if (t >= G16_CHAINS_G1 * g) return;
  const size_t proof = t / G16_CHAINS_G1;
  const int role = (int)(t % G16_CHAINS_G1);
  uint32_t rw[8], sw[8], k1[8], k2[8];
  load_words(d_r, proof, rw);
  load_words(d_s, proof, sw);
  g16_chain_scalars(role, rw, sw, k1, k2);
  uint32_t wa[16], wb[16], pw[16], qw[16];
  load_words(sa, 2 * proof, wa); load_words(sa, 2 * proof + 1, wa + 8);
  load_words(sb1, 2 * proof, wb); load_words(sb1, 2 * proof + 1, wb + 8);
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    pw[i] = role <= G16_ROLE_RS_DELTA ? vk.delta1[i] : (role == G16_ROLE_VK ? vk.alpha[i] : wa[i]);
    qw[i] = role == G16_ROLE_VK ? vk.beta1[i] : wb[i];
  }
  const bool p_inf = role == G16_ROLE_SUMS && sa_inf[proof] != 0;
  const bool q_inf = role <= G16_ROLE_RS_DELTA || (role == G16_ROLE_SUMS && sb1_inf[proof] != 0);
  const G16LdsOps<Fq> ops{lds + threadIdx.x};
  {
    const XYZZ<Fq> p = g16_g1_point(pw, p_inf), q = g16_g1_point(qw, q_inf);
    ops.put(0, p);
    ops.put(1, q);
    ops.put(2, add_xyzz(p, q));
  }
  const XYZZ<Fq> acc = g16_mul2_ops<Fq>(ops, k1, k2);
  PointIO<Fq>::store(chains, G16_CHAINS_G1 * g, t, acc);
}

// One lane per proof: the G2 chain s delta2 (role 4), then B = s delta2 + beta2 + Sb2 -> words 8 .. 23 of the proof and flag 1
__global__ void __launch_bounds__(G16_NT) k_g16_b_g2(G16VkG2 vk, const uint64_t* __restrict__ d_r, const uint64_t* __restrict__ d_s,
                                                     const uint64_t* __restrict__ sb2, const uint8_t* __restrict__ sb2_inf, size_t g,
                                                     uint64_t* __restrict__ proofs, uint8_t* __restrict__ inf) {
  __shared__ uint32_t lds[3 * PointIO<Fq2>::NW * G16_NT];
  const size_t proof = (size_t)blockIdx.x * G16_NT + threadIdx.x;
  if (proof >= g) return;
  uint32_t rw[8], sw[8], k1[8], k2[8];
  load_words(d_r, proof, rw);
  load_words(d_s, proof, sw);
  g16_chain_scalars(G16_ROLE_G2, rw, sw, k1, k2);
  const G16LdsOps<Fq2> ops{lds + threadIdx.x};
  {
    const XYZZ<Fq2> p = g16_g2_point(vk.delta2, false);
    ops.put(0, p);
    ops.put(1, XYZZ<Fq2>::identity());
    ops.put(2, p);
  }
  const XYZZ<Fq2> s_delta = g16_mul2_ops<Fq2>(ops, k1, k2);
  uint32_t w[32];
#pragma unroll
  for (int i = 0; i < 4; ++i) load_words(sb2, 4 * proof + i, w + 8 * i);
  const XYZZ<Fq2> b = g16_point_ab(s_delta, g16_g2_point(vk.beta2, false), g16_g2_point(w, sb2_inf[proof] != 0));
  put_affine_abi(b, proofs + proof * 32 + 8, inf + proof * 3 + 1);
}

// The finishing lane of a proof in G1: A = chain 0 + alpha + Sa -> words 0 .. 7, C = chains 1 + 2 + 3 + Sl + Sh -> words 24 .. 31
__global__ void __launch_bounds__(G16_NT) k_g16_finish_g1(G16VkG1 vk, const uint32_t* __restrict__ chains, const uint64_t* __restrict__ sa,
                                                          const uint8_t* __restrict__ sa_inf, const uint64_t* __restrict__ sl,
                                                          const uint8_t* __restrict__ sl_inf, const uint64_t* __restrict__ sh,
                                                          const uint8_t* __restrict__ sh_inf, size_t g, uint64_t* __restrict__ proofs,
                                                          uint8_t* __restrict__ inf) {
  const size_t proof = (size_t)blockIdx.x * G16_NT + threadIdx.x;
  if (proof >= g) return;
  const size_t lanes = G16_CHAINS_G1 * g, t0 = G16_CHAINS_G1 * proof;
  auto sum = [proof](const uint64_t* s, const uint8_t* f) {
    uint32_t w[16];
    load_words(s, 2 * proof, w); load_words(s, 2 * proof + 1, w + 8);
    return g16_g1_point(w, f[proof] != 0);
  };
  const XYZZ<Fq> a = g16_point_ab(PointIO<Fq>::load(chains, lanes, t0 + G16_ROLE_R_DELTA), g16_g1_point(vk.alpha, false), sum(sa, sa_inf));
  put_affine_abi(a, proofs + proof * 32, inf + proof * 3);
  const XYZZ<Fq> c = g16_point_c(PointIO<Fq>::load(chains, lanes, t0 + G16_ROLE_RS_DELTA), PointIO<Fq>::load(chains, lanes, t0 + G16_ROLE_VK),
                                 PointIO<Fq>::load(chains, lanes, t0 + G16_ROLE_SUMS), sum(sl, sl_inf), sum(sh, sh_inf));
  put_affine_abi(c, proofs + proof * 32 + 24, inf + proof * 3 + 2);
}

void vk_words(const uint64_t* src, int n64, uint32_t* dst) {
  for (int i = 0; i < n64; ++i) { dst[2 * i] = (uint32_t)src[i]; dst[2 * i + 1] = (uint32_t)(src[i] >> 32); }
}

bool len_ok(int curve, size_t len, size_t count) { return kg_commit_batch_plan(curve, len, count, nullptr) > 0; }

// one launch group: proofs [first, first + g) of the batch
struct G16BatchCall {
  const kg_groth16_crs* crs;
  const uint64_t *a, *b, *c, *x, *w, *r, *s;
  size_t eval_stride, x_stride, w_stride;
  uint64_t* proofs;
  uint8_t* inf;
  const kg_csr* mats[3];                                 // the R1CS form (kg_groth16_prove_r1cs_batch): a, b, c are null, the rows come from these
};
int g16_batch_group_run(kg_ctx* ctx, const G16BatchCall& q, size_t first, size_t g, char* ws, const Words8& zinv, const G16VkG1& vk1, const G16VkG2& vk2) {
  const kg_groth16_crs* crs = q.crs;
  const size_t m = crs->m, l = crs->l, m_l_1 = crs->m_l_1, nz = l + m_l_1, n = g16_batch_domain(m), hn = m - 1 < n ? m - 1 : n;
  const uint32_t k = g16_batch_log(m);
  const G16BatchLayout L = g16_batch_layout(g, n, nz);
  hipStream_t st = ctx->stream;
  uint64_t *A = (uint64_t*)(ws + L.poly), *B = A + 4 * g * n, *C = B + 4 * g * n, *Z = (uint64_t*)(ws + L.z);
  uint64_t *sa = (uint64_t*)(ws + L.sa), *sb1 = (uint64_t*)(ws + L.sb1), *sl = (uint64_t*)(ws + L.sl), *sh = (uint64_t*)(ws + L.sh), *sb2 = (uint64_t*)(ws + L.sb2);
  uint32_t* chains = (uint32_t*)(ws + L.chains);
  uint8_t *f_a = (uint8_t*)(ws + L.flags), *f_b1 = f_a + g, *f_l = f_b1 + g, *f_h = f_l + g, *f_b2 = f_h + g;
  {
    G16FillArgs fa;
    const bool evals = q.mats[0] == nullptr;
    const uint64_t* src[3] = {q.a, q.b, q.c};
    for (int v = 0; v < 3; ++v) fa.src[v] = evals ? src[v] + first * q.eval_stride * 4 : nullptr;
    fa.x = q.x + first * q.x_stride * 4;
    fa.w = q.w ? q.w + first * q.w_stride * 4 : nullptr;
    fa.eval_stride = q.eval_stride; fa.x_stride = q.x_stride; fa.w_stride = q.w_stride;
    fa.m = m; fa.l = l; fa.nz = nz; fa.n = n; fa.g = g; fa.dst = A;
    const size_t elems = g * (3 * n + nz);
    PhaseScope ph(ctx, "g16_batch_fill", st);
    hipLaunchKernelGGL(evals ? k_g16_fill<true> : k_g16_fill<false>, dim3((unsigned)((elems + 255) / 256)), dim3(256), 0, st, fa);
    ph.end();
    KG_HIP(ctx, hipGetLastError());
    if (!evals) {                                          // cs.evaluate() of the whole group: three batched products straight into the rows
      PhaseScope pe(ctx, "g16_batch_evaluate", st);
      uint64_t* rows[3] = {A, B, C};
      for (int v = 0; v < 3; ++v)
        KG_TRY(r1cs_prod_enqueue(ctx, st, KG_FR, q.mats[v]->d_row_ptr, q.mats[v]->d_col, q.mats[v]->d_val, m, Z, nz, g, rows[v], n,
                                 RowWs(ctx->ws_vec.get(), m, v)));
      pe.end();
    }
  }
  KG_TRY(kg_ntt_bn254_fr_batch(ctx, A, k, 3 * g, n, 1, 0));                 // idft, coset_dft of all rows (prover.rs:36-41)
  KG_TRY(kg_ntt_bn254_fr_batch(ctx, A, k, 3 * g, n, 0, 1));
  {
    PhaseScope pq(ctx, "g16_batch_combine", st);
    hipLaunchKernelGGL(k_qap_combine, dim3((unsigned)((g * n + 255) / 256)), dim3(256), 0, st, A, B, C, g * n, zinv);    // prover.rs:43-46
    pq.end();
    KG_HIP(ctx, hipGetLastError());
  }
  KG_TRY(kg_ntt_bn254_fr_batch(ctx, A, k, g, n, 1, 1));                     // coset_idft (prover.rs:47)
  // the eight MSMs of prover.rs:51-65 as five, like the single proof; a length of 0 writes identities
  KG_TRY(kg_commit_batch(ctx, KG_G1, crs->d_h, crs->d_h_inf, A, hn, g, n, sh, f_h));
  KG_TRY(kg_commit_batch(ctx, KG_G1, crs->d_a, crs->d_a_inf, Z, nz, g, nz, sa, f_a));
  KG_TRY(kg_commit_batch(ctx, KG_G1, crs->d_b_g1, crs->d_b_g1_inf, Z, nz, g, nz, sb1, f_b1));
  KG_TRY(kg_commit_batch(ctx, KG_G2, crs->d_b_g2, crs->d_b_g2_inf, Z, nz, g, nz, sb2, f_b2));
  KG_TRY(kg_commit_batch(ctx, KG_G1, crs->d_l, crs->d_l_inf, Z + 4 * l, m_l_1, g, nz, sl, f_l));
  // the assembly (prover.rs:75-92)
  const uint64_t *r = q.r + first * 4, *s = q.s + first * 4;
  uint64_t* proofs = q.proofs + first * 32;
  uint8_t* inf = q.inf + first * 3;
  PhaseScope pc(ctx, "g16_batch_chains_g1", st);
  hipLaunchKernelGGL(k_g16_chains_g1, dim3((unsigned)((G16_CHAINS_G1 * g + G16_NT - 1) / G16_NT)), dim3(G16_NT), 0, st, vk1, r, s, sa, f_a, sb1, f_b1, g, chains);
  pc.end();
  PhaseScope pb(ctx, "g16_batch_b_g2", st);
  hipLaunchKernelGGL(k_g16_b_g2, dim3((unsigned)((g + G16_NT - 1) / G16_NT)), dim3(G16_NT), 0, st, vk2, r, s, sb2, f_b2, g, proofs, inf);
  pb.end();
  PhaseScope pf(ctx, "g16_batch_finish_g1", st);
  hipLaunchKernelGGL(k_g16_finish_g1, dim3((unsigned)((g + G16_NT - 1) / G16_NT)), dim3(G16_NT), 0, st, vk1, chains, sa, f_a, sl, f_l, sh, f_h, g, proofs, inf);
  pf.end();
  KG_HIP(ctx, hipGetLastError());
  return KG_OK;
}

// both entries behind their argument checks; q.mats decides the form
int g16_batch_run(kg_ctx* ctx, const G16BatchCall& q, size_t count) {
  const kg_groth16_crs* crs = q.crs;
  const size_t m = crs->m, l = crs->l, m_l_1 = crs->m_l_1;
  if (crs->delta_g1_inf || crs->delta_g2_inf) return set_err(ctx, KG_ERR_CRS, "delta is the identity");      // prover.rs:67-69
  size_t per = 0;
  const size_t groups = g16_batch_plan(m, l, m_l_1, count, ctx->tune.g16_batch_mb, [count](int curve, size_t len) { return len_ok(curve, len, count); }, &per);
  if (groups == 0) return set_err(ctx, KG_ERR_UNSUPPORTED, "an MSM length of the circuit is outside the batched short MSM's (kg_commit_batch_plan)");
  KG_HIP(ctx, hipSetDevice(ctx->device));
  KG_TRY(ctx->ws_g16_batch.ensure(DevMem{ctx, "batched prover scratch"}, per * g16_batch_proof_bytes(m, l, m_l_1)));
  if (q.mats[0]) KG_TRY(ctx->ws_vec.ensure(DevMem{ctx, "workspace allocation"}, RowWs::bytes(m)));       // a work list per matrix, every group's
  const Words8 zinv = qap_zinv(g16_batch_log(m));
  G16VkG1 vk1;
  G16VkG2 vk2;
  vk_words(crs->alpha_g1, 8, vk1.alpha); vk_words(crs->beta_g1, 8, vk1.beta1); vk_words(crs->delta_g1, 8, vk1.delta1);
  vk_words(crs->beta_g2, 16, vk2.beta2); vk_words(crs->delta_g2, 16, vk2.delta2);
  for (size_t gi = 0; gi < groups; ++gi) {                  // one after another on the stream: every group uses the same scratch
    const G16BatchGroup grp = g16_batch_group(per, count, gi);
    KG_TRY(g16_batch_group_run(ctx, q, grp.first, grp.count, ctx->ws_g16_batch.as<char>(), zinv, vk1, vk2));
  }
  return KG_OK;
}
}  // namespace

extern "C" {

int kg_groth16_prove_batch_plan(size_t m, size_t l, size_t m_l_1, size_t count, size_t* per_group) {
  const size_t g = g16_batch_plan(m, l, m_l_1, count, tuning().g16_batch_mb, [count](int curve, size_t len) { return len_ok(curve, len, count); }, per_group);
  return g > (size_t)INT_MAX ? INT_MAX : (int)g;
}

int kg_groth16_prove_batch(kg_ctx* ctx, const kg_groth16_crs* crs, const uint64_t* d_a_eval, const uint64_t* d_b_eval, const uint64_t* d_c_eval,
                           size_t eval_stride, const uint64_t* d_x, size_t x_stride, const uint64_t* d_w, size_t w_stride, const uint64_t* d_r,
                           const uint64_t* d_s, size_t count, uint64_t* d_proofs, uint8_t* d_proof_inf) {
  return kg::kg_guarded(ctx, [&]() -> int {
  if (!ctx || !crs) return KG_ERR_BAD_ARG;
  if (!g16_batch_args_ok(ctx, crs, crs->m, crs->l, crs->m_l_1, d_a_eval, d_b_eval, d_c_eval, eval_stride, d_x, x_stride, d_w, w_stride, d_r, d_s, count, d_proofs,
                         d_proof_inf))
    return KG_ERR_BAD_ARG;
  if (count == 0) return KG_OK;
  return g16_batch_run(ctx, G16BatchCall{crs, d_a_eval, d_b_eval, d_c_eval, d_x, d_w, d_r, d_s, eval_stride, x_stride, w_stride, d_proofs, d_proof_inf,
                                         {nullptr, nullptr, nullptr}}, count);
  });
}

// The R1CS form: the constraint matrices instead of the three evaluation arrays.  The fill kernel zeroes the rows and builds z, three
// batched products (vec.hip) write A z, B z, C z of the whole group straight into the rows; from the transforms on it is the code above.
int kg_groth16_prove_r1cs_batch(kg_ctx* ctx, const kg_groth16_crs* crs, const kg_csr* a, const kg_csr* b, const kg_csr* c, const uint64_t* d_x,
                                size_t x_stride, const uint64_t* d_w, size_t w_stride, const uint64_t* d_r, const uint64_t* d_s, size_t count,
                                uint64_t* d_proofs, uint8_t* d_proof_inf) {
  return kg::kg_guarded(ctx, [&]() -> int {
  if (!ctx || !crs) return KG_ERR_BAD_ARG;
  if (!g16_r1cs_batch_args_ok(ctx, crs, crs->m, crs->l, crs->m_l_1, a, b, c, d_x, x_stride, d_w, w_stride, d_r, d_s, count, d_proofs, d_proof_inf))
    return KG_ERR_BAD_ARG;
  if (count == 0) return KG_OK;
  return g16_batch_run(ctx, G16BatchCall{crs, nullptr, nullptr, nullptr, d_x, d_w, d_r, d_s, crs->m, x_stride, w_stride, d_proofs, d_proof_inf, {a, b, c}}, count);
  });
}

}  // extern "C"
