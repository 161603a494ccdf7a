// points_fold.hip -- kg_points_muladd_batch: out_j = affine(P_j + k_{j / per_scalar} Q_j) for many points in one launch, results left on the
// device.  The instance fold of Nova's NIFS (nova/src/relaxed_r1cs/instance.rs:81-101: commit_w = commit_w1 + r commit_w2,
// commit_e = commit_e1 + r commit_T) for a batch of folds: the 2 count pairs interleaved, per_scalar = 2.
//
// One lane per point, one wave per workgroup.  The chain is the batched prover's (groth16_assemble.h g16_mul2_ops) with k1 = 1: the three
// operands P, Q and P + Q sit in LDS columns (chain_lds.h), per bit one doubling and at most one addition of the operand the two bits
// select -- bit 0 of k1 brings P in at the last step.  Lanes differ in data only; identities, P = Q and P = -Q go through the branches of
// add_xyzz / double_xyzz like every other lane.
#include "common.h"
#include "chain_lds.h"
#include "nova_batch.h"

using namespace kg;

namespace {

// F: the curve's base field, SP: its scalar field's parameters.  d_out_* may be d_p_*: a lane reads its own point before it writes it.
template <class F, class SP>
__global__ void __launch_bounds__(G16_NT) k_points_muladd(const uint64_t* p_xy, const uint8_t* p_inf, const uint64_t* __restrict__ q_xy,
                                                          const uint8_t* __restrict__ q_inf, const uint64_t* __restrict__ k, size_t per_scalar, size_t count,
                                                          uint64_t* out_xy, uint8_t* out_inf) {
  using P = typename F::Params;
  __shared__ uint32_t lds[3 * PointIO<F>::NW * G16_NT];
  const size_t j = (size_t)blockIdx.x * G16_NT + threadIdx.x;
  if (j >= count) return;
  uint32_t kw[8];
  load_words(k, points_muladd_scalar_at(j, per_scalar), kw);
  uint32_t pw[16], qw[16];
  load_words(p_xy, 2 * j, pw); load_words(p_xy, 2 * j + 1, pw + 8);
  load_words(q_xy, 2 * j, qw); load_words(q_xy, 2 * j + 1, qw + 8);
  const bool pi = p_inf != nullptr && p_inf[j] != 0, qi = q_inf != nullptr && q_inf[j] != 0;
  const G16LdsOps<F> ops{lds + threadIdx.x};
  {
    const XYZZ<F> p = g16_affine_point<P>(pw, pi), q = g16_affine_point<P>(qw, qi);
    ops.put(0, p);
    ops.put(1, q);
    ops.put(2, add_xyzz(p, q));
  }
  const XYZZ<F> acc = muladd_chain_ops<F, SP>(ops, kw);
  put_affine_abi(acc, out_xy + j * 8, out_inf + j);
}

}  // namespace

extern "C" {

int kg_points_muladd_batch(kg_ctx* c, int curve, const uint64_t* d_p_xy, const uint8_t* d_p_inf, const uint64_t* d_q_xy, const uint8_t* d_q_inf,
                           const uint64_t* d_k, size_t per_scalar, size_t count, uint64_t* d_out_xy, uint8_t* d_out_inf) {
  if (!points_muladd_args_ok(c, curve, d_p_xy, d_q_xy, d_k, per_scalar, count, d_out_xy, d_out_inf)) return KG_ERR_BAD_ARG;
  if (count == 0) return KG_OK;
  KG_HIP(c, hipSetDevice(c->device));
  const dim3 grid((unsigned)((count + G16_NT - 1) / G16_NT));
  if (curve == KG_G1)
    hipLaunchKernelGGL((k_points_muladd<Fq, FrParams>), grid, dim3(G16_NT), 0, c->stream, d_p_xy, d_p_inf, d_q_xy, d_q_inf, d_k, per_scalar, count, d_out_xy,
                       d_out_inf);
  else
    hipLaunchKernelGGL((k_points_muladd<Fr, FqParams>), grid, dim3(G16_NT), 0, c->stream, d_p_xy, d_p_inf, d_q_xy, d_q_inf, d_k, per_scalar, count, d_out_xy,
                       d_out_inf);
  KG_HIP(c, hipGetLastError());
  return KG_OK;
}

}  // extern "C"
