// host_point.h -- curve points between the ABI's words and the host field types (host_fp.h): what the host finish of an MSM (msm_host.cpp)
// and the proof assembly (groth16.hip) read and write.  Cfg: a configuration of curve_cfg.h.
#pragma once
#include "curve_cfg.h"
#include "curve.h"

namespace kg {

template <class HF> struct HostIO;
template <class P> struct HostIO<HostFp<P>> {
  static HostFp<P> load(const uint64_t* w) { return HostFp<P>::from_words(w); }
  static void store(const HostFp<P>& a, uint64_t* w) { a.to_words(w); }
};
template <class F> struct HostIO<Fp2<F>> {
  static Fp2<F> load(const uint64_t* w) { return {HostIO<F>::load(w), HostIO<F>::load(w + 4)}; }
  static void store(const Fp2<F>& a, uint64_t* w) { HostIO<F>::store(a.c0, w); HostIO<F>::store(a.c1, w + 4); }
};

// x | y (never the identity: the caller looks at the point's flag)
template <class Cfg>
Affine<typename Cfg::HF> host_load_affine(const uint64_t* p) {
  using HF = typename Cfg::HF;
  return {HostIO<HF>::load(p), HostIO<HF>::load(p + Cfg::E64)};
}
// x | y | zz | zzz: a window sum in a result slot
template <class Cfg>
XYZZ<typename Cfg::HF> host_load_point(const uint64_t* p) {
  using HF = typename Cfg::HF;
  constexpr int E = Cfg::E64;
  return {HostIO<HF>::load(p), HostIO<HF>::load(p + E), HostIO<HF>::load(p + 2 * E), HostIO<HF>::load(p + 3 * E)};
}

// affine x | y and flag; the identity is (0, 1) + flag 1: macros/curve/weierstrass/group.rs:22-26
template <class Cfg>
void store_affine(const XYZZ<typename Cfg::HF>& p, uint64_t* out_xy, uint8_t* out_inf) {
  using HF = typename Cfg::HF;
  Affine<HF> a;
  const bool finite = to_affine(p, a);
  HostIO<HF>::store(finite ? a.x : HF::zero(), out_xy);
  HostIO<HF>::store(finite ? a.y : HF::one(), out_xy + Cfg::E64);
  *out_inf = finite ? 0 : 1;
}
// (x, y, 1), the identity (0, 1, 0): macros/curve/weierstrass/group.rs:106-110
template <class Cfg>
void store_projective(const XYZZ<typename Cfg::HF>& p, uint64_t* out_xyz) {
  using HF = typename Cfg::HF;
  uint8_t inf;
  store_affine<Cfg>(p, out_xyz, &inf);
  HostIO<HF>::store(inf ? HF::zero() : HF::one(), out_xyz + 2 * Cfg::E64);
}

}  // namespace kg
