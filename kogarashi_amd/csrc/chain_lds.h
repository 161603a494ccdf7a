// chain_lds.h -- what the one-lane 255-step chain kernels share (groth16_batch.hip: the assembly of a batch of proofs; points_fold.hip:
// P + k Q for a batch of Nova folds): the chain's three operands in LDS columns and the loaders of an affine ABI point (the writer of
// the affine result is common.h's put_affine_abi).  The chain itself is g16_mul2_ops (groth16_assemble.h).  Device code: include after common.h.
#pragma once
#include "common.h"
#include "groth16_assemble.h"

namespace kg {

constexpr int G16_NT = 64;                               // one wave per workgroup: the chain kernels use no barrier

// the chain's three operands in LDS, one column per lane (word k of operand o at lds[(o * NW + k) * G16_NT + lane]: no bank conflicts)
template <class F>
struct G16LdsOps {
  static constexpr int NW = PointIO<F>::NW;
  uint32_t* col;                                         // lds + lane
  __device__ __forceinline__ void put(int o, const XYZZ<F>& p) const { PointIO<F>::store(col + (size_t)o * NW * G16_NT, G16_NT, 0, p); }
  __device__ __forceinline__ XYZZ<F> operator()(int sel) const { return PointIO<F>::load(col + (size_t)(sel - 1) * NW * G16_NT, G16_NT, 0); }
};

// affine x | y in ABI words and a flag -> the point (a base field of parameters P: G1 over Fq, Grumpkin over Fr)
template <class P>
__device__ __forceinline__ XYZZ<Fp<P>> g16_affine_point(const uint32_t w[16], bool inf) {
  if (inf) return XYZZ<Fp<P>>::identity();
  return from_affine(Affine<Fp<P>>{from_ref<P>(w), from_ref<P>(w + 8)});
}
__device__ __forceinline__ XYZZ<Fq> g16_g1_point(const uint32_t w[16], bool inf) { return g16_affine_point<FqParams>(w, inf); }
__device__ __forceinline__ XYZZ<Fq2> g16_g2_point(const uint32_t w[32], bool inf) {
  if (inf) return XYZZ<Fq2>::identity();
  return from_affine(Affine<Fq2>{{from_ref<FqParams>(w), from_ref<FqParams>(w + 8)}, {from_ref<FqParams>(w + 16), from_ref<FqParams>(w + 24)}});
}

}  // namespace kg
