// msm_small_finish.h -- the last step of a short MSM as a template over the field type: acc = sum_w 2^(c w) S_w over the W window sums the
// short kernel leaves (one point per window: msm_small_kernels.h "combine"), from the top window down -- c doublings and one addition per
// window, exactly the sl.combined loop of msm_finish_t (msm_host.cpp) -- then the affine point.  KG_HD: the finish kernel of the batched
// short MSM (msm_small_batch.hip) runs it with one lane per vector, tests/host/msm_batch_host.cpp compiles it for the host over the
// bound-tracking field type (fp29_checked.h) and over the host's own (host_fp.h).
#pragma once
#include "curve.h"

namespace kg {

// load(w): window sum S_w as an XYZZ point whose coordinates a curve formula accepts (normalised, < 2p)
template <class F, class Load>
KG_HD XYZZ<F> small_finish_chain(int W, int c, const Load& load) {
  XYZZ<F> acc = XYZZ<F>::identity();
  for (int w = W - 1; w >= 0; --w) {
    for (int l = 0; l < c; ++l) acc = double_xyzz(acc);
    acc = add_xyzz(acc, load(w));
  }
  return acc;
}

// the chain and the inversion (fp_inv.h, constant time); false: the sum is the identity and `out` is not written
template <class F, class Load>
KG_HD bool small_finish_affine(int W, int c, const Load& load, Affine<F>& out) {
  return to_affine(small_finish_chain<F>(W, c, load), out);
}

}  // namespace kg
