// curve_layout.h -- the ONE place that maps a curve id (KG_G1, KG_GRUMPKIN, KG_G2) to numbers: how many words a coordinate, a point and
// a resident base take, and which field the scalars live in.  Host-only and pure: no HIP, no context (tests/host/curve_layout_host.cpp
// includes this file alone).  The type side of a curve is curve_cfg.h; the two are asserted against each other there and in msm_common.h.
#pragma once
#include <cstddef>
#include "../../include/kogarashi_amd.h"

namespace kg {

constexpr bool curve_ok(int curve) { return curve == KG_G1 || curve == KG_GRUMPKIN || curve == KG_G2; }
// u64 words of the ABI: a coordinate (Fq, Fr: 4; Fq2: 8), an affine point (x | y), what kg_msm returns (x | y | z), one window sum in a
// result slot (x | y | zz | zzz)
constexpr size_t coord_words64(int curve) { return curve == KG_G2 ? 8 : 4; }
constexpr size_t affine_words64(int curve) { return 2 * coord_words64(curve); }
constexpr size_t projective_words64(int curve) { return 3 * coord_words64(curve); }
constexpr size_t xyzz_words64(int curve) { return 4 * coord_words64(curve); }
// u32 words of a base in its resident form: 64-byte points (fmt64; G2: 128 bytes) or nine 29-bit limbs per base-field element
constexpr size_t resident_words32(int curve, bool fmt64) { return coord_words64(curve) / 4 * (fmt64 ? 16 : 18); }
// u32 words of a raw XYZZ point in scratch memory (= PointIO<F>::NW)
constexpr size_t raw_xyzz_words32(int curve) { return coord_words64(curve) / 4 * 36; }
// the field of a curve's scalars: Grumpkin's is BN254's base field (nova/src/driver.rs:9-42)
constexpr int scalar_field(int curve) { return curve == KG_GRUMPKIN ? KG_FQ : KG_FR; }

}  // namespace kg
