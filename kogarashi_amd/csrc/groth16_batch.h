// groth16_batch.h -- the host-only, pure parts of the batched Groth16 prover (kg_groth16_prove_batch, groth16_batch.hip): the scratch one
// proof of a batch needs, how many proofs one launch group carries, where a group's arrays lie, and the argument checks.  No HIP, no
// context: tests/host/g16_batch_host.cpp includes this file alone.
//
// Layout of a launch group of g proofs in the context's grow-only scratch (n = max(2, next power of two of m), nz = l + m_l_1):
//   [3][g][n]   the padded polynomials, all a rows, then all b rows, then all c rows (32-byte elements): the batched transform runs over
//               3 g rows of stride n, the point-wise step over the g n contiguous elements of a, b and c, h's MSM over row a, stride n
//   [g][nz]     z = x || w
//   the points  per proof G16_BATCH_POINT_BYTES: the five sums as kg_commit_batch writes them (four G1 points of 64 bytes, one G2 point
//               of 128), the four G1 chain results in raw limbs (4 x 144 bytes) and the five identity flags
// Groups run one after another on the stream over the same scratch.
#pragma once
#include <climits>
#include <cstddef>
#include <cstdint>

namespace kg {

constexpr size_t G16_BATCH_POINT_BYTES = 1024;        // 4 x 64 + 128 + 4 x 144 + 5 flags = 965, rounded up
constexpr size_t G16_BATCH_MAX_LOG = 28;              // the transform's limit (kg_ntt_bn254_fr_batch)
constexpr int G16_BATCH_MB_MIN = 1, G16_BATCH_MB_MAX = 4096;   // range of KG_G16_BATCH_MB (tuning.h)
constexpr int G16_CHAINS_G1 = 4;                      // G1 chains of a proof (groth16_assemble.h)

// n = max(2, m.next_power_of_two()) (prover.rs:28-29); m <= 2^28
inline size_t g16_batch_domain(size_t m) {
  size_t n = 2;
  while (n < m) n <<= 1;
  return n;
}
inline uint32_t g16_batch_log(size_t m) {
  uint32_t k = 1;
  while (((size_t)1 << k) < m) ++k;
  return k;
}
inline size_t g16_batch_cap_bytes(int mb) {
  const int c = mb < G16_BATCH_MB_MIN ? G16_BATCH_MB_MIN : (mb > G16_BATCH_MB_MAX ? G16_BATCH_MB_MAX : mb);
  return (size_t)c << 20;
}
// do the three lengths describe a circuit the call accepts at all (KG_ERR_BAD_ARG otherwise), with every size below in a size_t?
inline bool g16_batch_shape_ok(size_t m, size_t l, size_t m_l_1) {
  if (m < 1 || l < 1 || m > ((size_t)1 << G16_BATCH_MAX_LOG)) return false;
  if (l > SIZE_MAX / 64 || m_l_1 > SIZE_MAX / 64) return false;                    // (l + m_l_1) * 32
  return true;
}
// scratch bytes of one proof (shape_ok)
inline size_t g16_batch_proof_bytes(size_t m, size_t l, size_t m_l_1) {
  return (3 * g16_batch_domain(m) + l + m_l_1) * 32 + G16_BATCH_POINT_BYTES;
}
// THE group rule: min(count, cap / scratch bytes per proof), at least 1 (0 for an empty batch)
inline size_t g16_batch_per_group(size_t proof_bytes, size_t cap_bytes, size_t count) {
  if (count == 0) return 0;
  size_t per = cap_bytes / proof_bytes;
  if (per < 1) per = 1;
  return per < count ? per : count;
}
inline size_t g16_batch_groups(size_t per_group, size_t count) { return per_group == 0 || count == 0 ? 0 : (count - 1) / per_group + 1; }
struct G16BatchGroup { size_t first, count; };
inline G16BatchGroup g16_batch_group(size_t per_group, size_t count, size_t g) {
  const size_t first = g * per_group;
  return {first, count - first < per_group ? count - first : per_group};
}
// The MSM lengths of a proof: a, b_g1 (G1) and b_g2 (G2) meet z, l meets w, h meets the m - 1 low coefficients.  len_ok(curve, len): does
// the batched short MSM run vectors of this length batched (kg_commit_batch_plan > 0)?  Zero lengths write identities and are always taken.
template <class LenOk>
inline bool g16_batch_lengths_ok(size_t m, size_t l, size_t m_l_1, const LenOk& len_ok) {
  const size_t nz = l + m_l_1, n = g16_batch_domain(m), hn = m - 1 < n ? m - 1 : n;
  if (!len_ok(0, nz) || !len_ok(2, nz)) return false;
  if (m_l_1 && !len_ok(0, m_l_1)) return false;
  if (hn && !len_ok(0, hn)) return false;
  return true;
}
// kg_groth16_prove_batch_plan: the number of groups, *per_group = proofs of a full group; 0 / 0 for an empty batch, a shape the call
// refuses and lengths outside the batched MSM's
template <class LenOk>
inline size_t g16_batch_plan(size_t m, size_t l, size_t m_l_1, size_t count, int cap_mb, const LenOk& len_ok, size_t* per_group) {
  if (per_group) *per_group = 0;
  if (count == 0 || !g16_batch_shape_ok(m, l, m_l_1) || !g16_batch_lengths_ok(m, l, m_l_1, len_ok)) return 0;
  const size_t per = g16_batch_per_group(g16_batch_proof_bytes(m, l, m_l_1), g16_batch_cap_bytes(cap_mb), count);
  if (per_group) *per_group = per;
  return g16_batch_groups(per, count);
}

// byte offsets of a group's arrays in the scratch (g proofs, domain n, nz = l + m_l_1)
struct G16BatchLayout {
  size_t poly, z, sa, sb1, sl, sh, sb2, chains, flags, bytes;
};
inline G16BatchLayout g16_batch_layout(size_t g, size_t n, size_t nz) {
  G16BatchLayout L;
  L.poly = 0;
  L.z = 3 * g * n * 32;
  L.sa = L.z + g * nz * 32;
  L.sb1 = L.sa + g * 64;
  L.sl = L.sb1 + g * 64;
  L.sh = L.sl + g * 64;
  L.sb2 = L.sh + g * 64;
  L.chains = L.sb2 + g * 128;
  L.flags = L.chains + g * G16_CHAINS_G1 * 144;       // five arrays of g flags: a, b1, l, h, b2
  L.bytes = g * ((3 * n + nz) * 32 + G16_BATCH_POINT_BYTES);
  return L;
}

// The argument checks of kg_groth16_prove_batch (true = acceptable), made before anything is dereferenced; m, l, m_l_1 are the CRS's (read
// once ctx and crs are known not to be null).  count == 0 is acceptable with any array pointers.
inline bool g16_batch_args_ok(const void* ctx, const void* crs, size_t m, size_t l, size_t m_l_1, const void* d_a, const void* d_b, const void* d_c,
                              size_t eval_stride, const void* d_x, size_t x_stride, const void* d_w, size_t w_stride, const void* d_r, const void* d_s,
                              size_t count, const void* d_proofs, const void* d_inf) {
  if (!ctx || !crs || !g16_batch_shape_ok(m, l, m_l_1)) return false;
  if (eval_stride < m || x_stride < l || w_stride < m_l_1) return false;
  if (count == 0) return true;
  if (!d_a || !d_b || !d_c || !d_x || !d_r || !d_s || !d_proofs || !d_inf) return false;
  if (m_l_1 && !d_w) return false;
  if (count > SIZE_MAX / 256) return false;                                          // count proofs of 32 words
  if (eval_stride > SIZE_MAX / 32 / count || x_stride > SIZE_MAX / 32 / count || w_stride > SIZE_MAX / 32 / count) return false;
  return true;
}

}  // namespace kg
