// points.hip -- kg_points_check / kg_groth16_crs_check: curve points validated on the device before they are trusted (registered as MSM
// bases, used as a CRS).  The predicates are points_check.h's (shared with the host twin of tests/host/points_check_host.cpp); this file
// holds the two kernels around them and the entry points.
//
//   k_points_check<F, false>   canonical words + curve equation, one lane per point, one pass: 64 B (G1, Grumpkin) or 128 B (G2) read per
//                              point, a dozen field products -- bound by memory on G1.
//   k_points_check<Fq2, true>  the same, then the order-r test of the twist for the lanes that passed (points_check.h: ~95 point operations
//                              on XYZZ<Fq2>, the register footprint of k_acc_tasks<Fq2>).
// Both write the status byte and fold the summary in the same launch: per 64-lane workgroup one ballot, one 64-bit atomicAdd of the popcount
// and one 64-bit atomicMin of the lowest bad index, into two words of the context that k_summary_init (common.h) sets to (0, n) on the stream first.
#include "msm_common.h"
#include "points_check.h"

using namespace kg;

static_assert(pts::ST_NON_CANONICAL == KG_PT_NON_CANONICAL && pts::ST_OFF_CURVE == KG_PT_OFF_CURVE && pts::ST_NOT_IN_SUBGROUP == KG_PT_NOT_IN_SUBGROUP,
              "points_check.h status bits are the public header's");

namespace {

constexpr size_t WS_SUMMARY = 16;                               // bad count | first bad index
constexpr size_t WS_HOST_XY = (3 * 8 + 2 * 16) * 8;             // the five host points of a CRS: alpha_g1 | beta_g1 | delta_g1 | beta_g2 | delta_g2
constexpr size_t WS_BYTES = WS_SUMMARY + WS_HOST_XY + 16;       // + their flags

// 64-lane workgroups: the subgroup chain keeps an XYZZ<Fq2> accumulator, the affine point and the temporaries of an addition live, and a
// one-wave workgroup lets the compiler take what it needs of the register file (VGPRs + AGPRs) before it reaches for scratch memory
template <class F, bool SUB>
__global__ void __launch_bounds__(64) k_points_check(const uint64_t* __restrict__ xy, const uint8_t* __restrict__ inf, size_t n, uint8_t* __restrict__ status,
               unsigned long long* __restrict__ summary) {
  constexpr int NW = pts::Coord<F>::NW;                         // u32 words per coordinate = u64 words per point
  const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
  uint8_t st = 0;
  if (i < n) {
    const bool identity = inf != nullptr && inf[i] != 0;        // the flag rule of k_prep_bases (msm_bases.h)
    if (!identity) {
      uint32_t w[2 * NW];
#pragma unroll
      for (int e = 0; e < NW / 4; ++e) load_words(xy, i * (NW / 4) + e, w + 8 * e);
      st = pts::point_status<F, SUB>(w, false);
    }
    if (status) status[i] = st;
  }
  // 64-lane workgroup = one wave; thread 0 speaks for it (summary_fold's lowest bad lane changes the subgroup kernel's register split: 133 AGPRs for 134)
  const unsigned long long bad = __ballot(st != 0);
  if (bad != 0 && threadIdx.x == 0)
    summary_add(summary, (unsigned long long)__popcll(bad), (unsigned long long)blockIdx.x * 64 + (unsigned long long)(__ffsll((long long)bad) - 1));
}

template <class F, bool SUB>
void launch_check(kg_ctx* c, const uint64_t* xy, const uint8_t* inf, size_t n, uint8_t* status, unsigned long long* summary) {
  hipLaunchKernelGGL((k_points_check<F, SUB>), dim3((unsigned)((n + 63) / 64)), dim3(64), 0, c->stream, xy, inf, n, status, summary);
}

// enqueue + read back; arguments are checked by the callers
int run_check(kg_ctx* c, int curve, const uint64_t* d_xy, const uint8_t* d_inf, size_t n, int checks, uint8_t* d_status, size_t* out_bad,
              size_t* out_first_bad) {
  if (n == 0) {
    if (out_bad) *out_bad = 0;
    if (out_first_bad) *out_first_bad = 0;
    return KG_OK;
  }
  if (n >= ((size_t)1 << 37)) return set_err(c, KG_ERR_BAD_ARG, "more than 2^37 points");       // the grid's x dimension
  KG_TRY(c->ws_points.ensure(DevMem{c, "point-check work space"}, WS_BYTES));
  unsigned long long* summary = c->ws_points.as<unsigned long long>();
  hipLaunchKernelGGL(k_summary_init<unsigned long long>, dim3(1), dim3(1), 0, c->stream, summary, (unsigned long long)n);
  const bool sub = (checks & KG_CHECK_SUBGROUP) != 0;
  with_curve(curve, [&](auto cfg) {                            // the order-r test exists for the twist alone (G1, Grumpkin: cofactor 1)
    using F = typename CurveDev<decltype(cfg)>::F;
    if constexpr (decltype(cfg)::ID == KG_G2) { if (sub) return launch_check<F, true>(c, d_xy, d_inf, n, d_status, summary); }
    launch_check<F, false>(c, d_xy, d_inf, n, d_status, summary);
  });
  KG_HIP(c, hipGetLastError());
  return summary_read(c, summary, out_bad, out_first_bad);
}

bool checks_ok(int checks) { return checks != 0 && (checks & ~(KG_CHECK_CURVE | KG_CHECK_SUBGROUP)) == 0; }

}  // namespace

extern "C" {

int kg_points_check(kg_ctx* c, int curve, const uint64_t* d_xy, const uint8_t* d_inf, size_t n, int checks, uint8_t* d_status, size_t* out_bad,
                    size_t* out_first_bad) {
  if (!c || !curve_ok(curve) || !checks_ok(checks)) return KG_ERR_BAD_ARG;
  if (n > 0 && !d_xy) return KG_ERR_BAD_ARG;
  KG_HIP(c, hipSetDevice(c->device));
  return run_check(c, curve, d_xy, d_inf, n, checks, d_status, out_bad, out_first_bad);
}

int kg_groth16_crs_check(kg_ctx* c, const kg_groth16_crs* crs, int checks, size_t* out_bad) {
  if (!c || !crs || !out_bad || !checks_ok(checks)) return KG_ERR_BAD_ARG;
  const size_t n_h = crs->m > 0 ? crs->m - 1 : 0, n_l = crs->m_l_1, n_q = crs->l + crs->m_l_1;
  struct Member { int curve; const uint64_t* xy; const uint8_t* inf; size_t n; };
  const Member dev[5] = {{KG_G1, crs->d_h, crs->d_h_inf, n_h}, {KG_G1, crs->d_l, crs->d_l_inf, n_l}, {KG_G1, crs->d_a, crs->d_a_inf, n_q},
                         {KG_G1, crs->d_b_g1, crs->d_b_g1_inf, n_q}, {KG_G2, crs->d_b_g2, crs->d_b_g2_inf, n_q}};
  for (const Member& m : dev)
    if (m.n > 0 && !m.xy) return KG_ERR_BAD_ARG;
  KG_HIP(c, hipSetDevice(c->device));
  for (int k = 0; k < 10; ++k) out_bad[k] = 0;
  for (int k = 0; k < 5; ++k) KG_TRY(run_check(c, dev[k].curve, dev[k].xy, dev[k].inf, dev[k].n, checks, nullptr, &out_bad[k], nullptr));
  // the five host points, through a small device buffer of the context
  KG_TRY(c->ws_points.ensure(DevMem{c, "point-check work space"}, WS_BYTES));
  uint64_t h_xy[WS_HOST_XY / 8];
  uint8_t h_inf[16] = {0};
  for (int i = 0; i < 8; ++i) { h_xy[i] = crs->alpha_g1[i]; h_xy[8 + i] = crs->beta_g1[i]; h_xy[16 + i] = crs->delta_g1[i]; }
  for (int i = 0; i < 16; ++i) { h_xy[24 + i] = crs->beta_g2[i]; h_xy[40 + i] = crs->delta_g2[i]; }
  h_inf[2] = crs->delta_g1_inf;
  h_inf[4] = crs->delta_g2_inf;
  uint64_t* d_xy = (uint64_t*)(c->ws_points.as<char>() + WS_SUMMARY);
  uint8_t* d_inf = c->ws_points.as<uint8_t>() + WS_SUMMARY + WS_HOST_XY;
  KG_HIP(c, hipMemcpyAsync(d_xy, h_xy, sizeof h_xy, hipMemcpyHostToDevice, c->stream));
  KG_HIP(c, hipMemcpyAsync(d_inf, h_inf, sizeof h_inf, hipMemcpyHostToDevice, c->stream));
  KG_HIP(c, hipStreamSynchronize(c->stream));
  for (int k = 0; k < 3; ++k) KG_TRY(run_check(c, KG_G1, d_xy + 8 * k, d_inf + k, 1, checks, nullptr, &out_bad[5 + k], nullptr));
  for (int k = 0; k < 2; ++k) KG_TRY(run_check(c, KG_G2, d_xy + 24 + 16 * k, d_inf + 3 + k, 1, checks, nullptr, &out_bad[8 + k], nullptr));
  return KG_OK;
}

}  // extern "C"
