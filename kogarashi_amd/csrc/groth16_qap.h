// groth16_qap.h -- the point-wise step of the Groth16 prover, shared by the single proof (groth16.hip) and the batched one
// (groth16_batch.hip): h = (a o b - c) / Z on the coset (prover.rs:43-46), and the constant it divides by.
#pragma once
#include "common.h"
#include "host_fp.h"

namespace kg {

// h[i] = (a[i] * b[i] - c[i]) * zinv   (poly.rs:168-195 + fft.rs:150-154 in one pass; data stays in ABI form)
static __global__ void __launch_bounds__(256) k_qap_combine(uint64_t* __restrict__ a, const uint64_t* __restrict__ b, const uint64_t* __restrict__ c,
                                                            size_t n, Words8 zinv) {
  KG_SERVICE_PRIO();
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t wa[8], wb[8], wc[8], wo[8];
  load_words(a, i, wa); load_words(b, i, wb); load_words(c, i, wc);
  Fr x = from_ref<FrParams>(wa), y = from_ref<FrParams>(wb), z = from_ref<FrParams>(wc);
  Fr t = norm(sub<4, 1>(mul(x, y), z));
  to_ref(mul(t, from_ref<FrParams>(zinv.w)), wo);
  store_words(a, i, wo);
}

// (7^n - 1)^-1 for n = 2^k on the host: k squarings of 7, z_on_coset().invert() (fft.rs:141-151)
inline Words8 qap_zinv(uint32_t k) {
  HostFr one = HostFr::one(), z = HostFr::zero();
  for (int i = 0; i < 7; ++i) z = add(z, one);
  for (uint32_t i = 0; i < k; ++i) z = sqr(z);
  z = inv(sub<4, 1>(z, HostFr::one()));
  return words8(z.v);
}

}  // namespace kg
