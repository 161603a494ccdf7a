// curve_cfg.h -- the type side of a curve, once: the host field of its coordinates, and the one dispatcher from a run-time curve id to
// a configuration.  Host code (msm_host.cpp, host_point.h) uses the configurations as they are; device code adds the device's field types
// through CurveDev<Cfg> (msm_common.h).  The numbers of a curve are curve_layout.h's.
#pragma once
#include <cassert>
#include <type_traits>
#include "curve_layout.h"
#include "host_fp.h"

namespace kg {

struct G1Cfg { using HF = HostFq; static constexpr int E64 = 4; static constexpr int ID = KG_G1; };
struct GkCfg { using HF = HostFr; static constexpr int E64 = 4; static constexpr int ID = KG_GRUMPKIN; };
struct G2Cfg { using HF = HostFq2; static constexpr int E64 = 8; static constexpr int ID = KG_G2; };
static_assert(G1Cfg::E64 == coord_words64(G1Cfg::ID) && GkCfg::E64 == coord_words64(GkCfg::ID) && G2Cfg::E64 == coord_words64(G2Cfg::ID),
              "curve_cfg.h: a configuration's coordinate words are curve_layout.h's");

// f(G1Cfg{}), f(GkCfg{}) or f(G2Cfg{}) by the curve id (f: a generic lambda).  Any other id: KG_ERR_BAD_ARG -- or, where f returns nothing
// (a helper behind an entry point that has checked the id), an assertion.
template <class Fn>
inline auto with_curve(int curve, Fn&& f) -> decltype(f(G1Cfg{})) {
  switch (curve) {
    case KG_G1: return f(G1Cfg{});
    case KG_GRUMPKIN: return f(GkCfg{});
    case KG_G2: return f(G2Cfg{});
  }
  if constexpr (std::is_void<decltype(f(G1Cfg{}))>::value) assert(!"with_curve: unknown curve id");
  else return KG_ERR_BAD_ARG;
}

}  // namespace kg
