// devprobe_reduce.h -- TEST-ONLY entries of libdevprobe.so (included by devprobe.hip) for the point-side kernels of the long MSM: the
// conversion of the bases and their window tables (msm_bases.h), the accumulation and the bucket gather (msm_acc_kernels.h), and the gathers,
// the further partial-sum round, the halving level, the fused tails and the hot-bucket trees of msm_reduce_kernels.h -- included unchanged
// and launched ONE AT A TIME on buffers and tables the caller built (tests/reduce_cases.py: the reference's tables and points, never the
// output of an earlier launch).  Nothing here restates product arithmetic.
//
// The conventions are those of devprobe_sort.h:  int dp_xxx(const KBuf* b, const int64_t* p), b the HOST arrays (uploaded whole; an `io`
// buffer is copied back whole, guard region included), p the scalar parameters.  Result: the first HIP status that was not hipSuccess
// (0: ok), -1 for a parameter the kernel is not built for, -2 for a table or buffer that would let the launch touch memory outside what
// the caller passed -- looked at on the HOST copies before anything is launched (only ranges: not a check of the kernels).  Every buffer
// an entry lists must be given.  Grid, block, dynamic LDS and function attributes are those msm_run.hip uses for the kernel.
// p[0] is always the curve: 0 G1 (Fq), 1 Grumpkin (Fr), 2 G2 (Fq2; lane pairs Fp2S<Fq> where the product launches the kernel on them).
#pragma once
#include "devprobe_sort.h"
#include "../../kogarashi_amd/csrc/msm_reduce_kernels.h"

namespace reduceprobe {
using namespace kg;
using namespace kg::msm;
using sortprobe::Dev;
using sortprobe::KBuf;

inline const uint32_t* hw(const KBuf* b, int i) { return (const uint32_t*)b[i].host; }
inline bool given(const KBuf* b, int n) { for (int i = 0; i < n; ++i) if (!b[i].host) return false; return true; }
inline int log2u(uint32_t v) { int s = 0; while ((1u << s) < v) ++s; return s; }
inline bool pow2(uint32_t v) { return v && !(v & (v - 1)); }
constexpr uint64_t SPAN = (uint64_t)1 << 32;           // byte offsets are 32-bit lane offsets of one buffer descriptor

// dense bucket array from the partial sums.  which: 0 k_gather_buckets<F>, 1 k_gather_halve<KF>, 2 k_gather_sum<F, KF>
template <class Cfg>
int gather(const KBuf* b, const int64_t* p) {
  using F = typename Cfg::F; using KF = typename Cfg::KF;
  constexpr uint32_t NW = (uint32_t)PointIO<F>::NW, LPT = (uint32_t)Lanes<KF>::N;
  const int which = (int)p[1], W = (int)p[2], B = (int)p[3];
  const uint64_t cap = (uint64_t)p[4];
  if (which < 0 || which > 2 || W < 1 || B < 1 || (uint64_t)W * B > ((uint64_t)1 << 20) || p[4] < 1 || cap * NW * 4 >= SPAN || (which == 1 && (B & 1))) return -1;
  if (!given(b, 5)) return -2;
  const size_t npts = (size_t)W * B;
  Dev D(b, 5);
  SP_NEED(0, cap * NW); SP_NEED(1, npts); SP_NEED(2, npts); SP_NEED(3, W + 1); SP_NEED(4, npts * NW);
  const uint32_t *cnt = hw(b, 1), *rel = hw(b, 2), *base = hw(b, 3);
  for (size_t t = 0; t < npts; ++t) {
    if (!cnt[t]) continue;
    const uint64_t take = which == 2 && cnt[t] <= GATHER_SUM_MAX ? cnt[t] : 1;
    if ((uint64_t)base[t / B] + rel[t] + take > cap) return -2;
  }
  const Level L{D.u(1), D.u(2), D.u(3)};
  if (D.ok()) {
    if (which == 0) hipLaunchKernelGGL(k_gather_buckets<F>, dim3((unsigned)((npts + 255) / 256)), dim3(256), 0, 0, D.u(0), (size_t)cap, L, W, B, D.u(4));
    else if (which == 1) hipLaunchKernelGGL(k_gather_halve<KF>, dim3((unsigned)((npts / 2 * LPT + 63) / 64)), dim3(64), 0, 0, D.u(0), L, W, B, D.u(4), (size_t)W * 2 * (B / 2));
    else hipLaunchKernelGGL((k_gather_sum<F, KF>), dim3((unsigned)((npts * LPT + 63) / 64)), dim3(64), 0, 0, D.u(0), L, W, B, D.u(4));
  }
  return D.finish();
}

template <class Cfg>
int sum_tasks(const KBuf* b, const int64_t* p) {
  using KF = typename Cfg::KF;
  constexpr uint32_t NW = (uint32_t)PointIO<KF>::NW, LPT = (uint32_t)Lanes<KF>::N;
  const int W = (int)p[1], B = (int)p[2];
  const uint64_t T2 = (uint64_t)p[3], bound = (uint64_t)p[4], in_cap = (uint64_t)p[5], out_cap = (uint64_t)p[6];
  if (W < 1 || B < 1 || (uint64_t)W * B > ((uint64_t)1 << 20) || p[3] < 1 || p[3] > (1 << 20) || p[4] < 1 || p[5] < 1 || p[6] < 1 || in_cap * NW * 4 >= SPAN ||
      out_cap * NW * 4 >= SPAN || bound * LPT >= SPAN)
    return -1;
  if (!given(b, 8)) return -2;
  const size_t npts = (size_t)W * B;
  Dev D(b, 8);
  SP_NEED(0, in_cap * NW); SP_NEED(1, npts); SP_NEED(2, npts); SP_NEED(3, W + 1); SP_NEED(4, npts); SP_NEED(5, npts); SP_NEED(6, W + 1); SP_NEED(7, out_cap * NW);
  // the new level must be the exclusive scans of its own counters (locate_task then lands on a bucket that has the task), every task must
  // start inside its bucket's previous partial sums, and those must lie inside pin
  const uint32_t *ci = hw(b, 1), *ri = hw(b, 2), *bi_ = hw(b, 3), *co = hw(b, 4), *ro = hw(b, 5), *bo = hw(b, 6);
  uint64_t run = 0;
  for (int w = 0; w < W; ++w) {
    if (bo[w] != run) return -2;
    uint64_t r = 0;
    for (int k = 0; k < B; ++k) {
      const size_t t = (size_t)w * B + k;
      if (ro[t] != r) return -2;
      if (co[t]) {
        if ((uint64_t)(co[t] - 1) * T2 >= ci[t] || (uint64_t)bi_[w] + ri[t] + ci[t] > in_cap) return -2;
        r += co[t];
      }
    }
    run += r;
  }
  if (bo[W] != run || run > out_cap || run >= SPAN) return -2;
  const Level Lin{D.u(1), D.u(2), D.u(3)}, L{D.u(4), D.u(5), D.u(6)};
  if (D.ok()) hipLaunchKernelGGL(k_sum_tasks<KF>, dim3((unsigned)((bound * LPT + 63) / 64)), dim3(64), 0, 0, D.u(0), Lin, L, W, B, (uint32_t)T2, D.u(7));
  return D.finish();
}

template <class Cfg>
int halve(const KBuf* b, const int64_t* p) {
  using KF = typename Cfg::KF;
  constexpr uint32_t NW = (uint32_t)PointIO<KF>::NW, LPT = (uint32_t)Lanes<KF>::N;
  const int W = (int)p[1], narr = (int)p[2];
  const uint64_t n_out = (uint64_t)p[3], is = (uint64_t)p[4], os = (uint64_t)p[5];
  if (W < 1 || W > 64 || narr < 1 || narr > 32 || p[3] < 1 || p[3] > (1 << 17) || p[4] < 1 || p[5] < 1 || is * NW * 4 >= SPAN || os * NW * 4 >= SPAN) return -1;
  if (!given(b, 2)) return -2;
  if (is < (uint64_t)W * narr * 2 * n_out || os < (uint64_t)W * (narr + 1) * n_out) return -2;
  Dev D(b, 2);
  SP_NEED(0, is * NW); SP_NEED(1, os * NW);
  const size_t tasks = (size_t)W * narr * n_out;
  if (D.ok()) hipLaunchKernelGGL(k_halve<KF>, dim3((unsigned)((tasks * LPT + 63) / 64)), dim3(64), 0, 0, D.u(0), (size_t)is, D.u(1), (size_t)os, W, narr, (uint32_t)n_out);
  return D.finish();
}

// form: 0 k_reduce_tail<KF, E64, TL> (len = TL), 1 k_reduce_tail<KF, E64, 0> (len <= TL / 2), 2 k_reduce_tail_coop<F, E64>
template <class Cfg>
int reduce_tail(const KBuf* b, const int64_t* p) {
  using F = typename Cfg::F; using KF = typename Cfg::KF;
  constexpr uint32_t NW = (uint32_t)PointIO<KF>::NW, LPT = (uint32_t)Lanes<KF>::N, TL = (uint32_t)TailCfg<KF>::L;
  constexpr int E64 = Cfg::E64;
  const int form = (int)p[1], W = (int)p[2], narr = (int)p[3], c = (int)p[5];
  const uint64_t is = (uint64_t)p[6];
  if (form < 0 || form > 2 || W < 1 || W > 64 || narr < 1 || narr > 32 || p[4] < 2 || p[4] > (int64_t)TL || p[6] < 1 || is * NW * 4 >= SPAN || c < 1 || c > 64) return -1;
  const uint32_t len = (uint32_t)p[4];
  if (!pow2(len) || (form == 0 && len != TL) || (form == 1 && len > TL / 2)) return -1;
  if (!given(b, 2)) return -2;
  if (narr + log2u(len) > c || is < (uint64_t)W * narr * len) return -2;          // the last array's slot is (w * c + narr - 1 + log2 len)
  Dev D(b, 2);
  SP_NEED(0, is * NW); SP_NEED(1, (uint64_t)W * c * 4 * E64 * 2);
  const unsigned grid = (unsigned)(W * narr);
  const unsigned tail_threads = (unsigned)(len / 2 * LPT) < 64u ? 64u : (unsigned)(len / 2 * LPT);
  if (form == 2) {
    const size_t lds = tail_coop_lds_bytes<F>(len);
    if (lds > 160 * 1024) return -1;
    D.keep(hipFuncSetAttribute((const void*)(k_reduce_tail_coop<F, E64>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    if (D.ok()) hipLaunchKernelGGL((k_reduce_tail_coop<F, E64>), dim3(grid), dim3(TailCoopNT<F>::NT), lds, 0, D.u(0), (size_t)is, narr, len, c, D.at<uint64_t>(1));
  } else if (form == 0) {
    const size_t lds = tail_lds_bytes(len, (int)LPT);
    D.keep(hipFuncSetAttribute((const void*)(k_reduce_tail<KF, E64, (int)TL>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    if (D.ok()) hipLaunchKernelGGL((k_reduce_tail<KF, E64, (int)TL>), dim3(grid), dim3(tail_threads), lds, 0, D.u(0), (size_t)is, narr, len, c, D.at<uint64_t>(1));
  } else {
    const size_t lds0 = tail_lds_bytes(TL / 2, (int)LPT);
    D.keep(hipFuncSetAttribute((const void*)(k_reduce_tail<KF, E64, 0>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds0));
    if (D.ok()) hipLaunchKernelGGL((k_reduce_tail<KF, E64, 0>), dim3(grid), dim3(tail_threads), lds0, 0, D.u(0), (size_t)is, narr, len, c, D.at<uint64_t>(1));
  }
  return D.finish();
}

// which: 0 k_hot_sum<KF> (grid nhot x split), 1 k_hot_fold<KF> (grid nhot)
template <class Cfg>
int hot(const KBuf* b, const int64_t* p) {
  using KF = typename Cfg::KF;
  constexpr uint32_t NW = (uint32_t)PointIO<KF>::NW;
  const int which = (int)p[1], B = (int)p[2], W = (int)p[5];
  const uint64_t nhot = (uint64_t)p[3], split = (uint64_t)p[4], cap = (uint64_t)p[6];
  if (which < 0 || which > 1 || B < 1 || W < 1 || (uint64_t)W * B > ((uint64_t)1 << 20) || p[3] < 1 || nhot > HOT_MAX || p[4] < 1 || split > hot_split_max<KF>() || p[6] < 1 ||
      cap * NW * 4 >= SPAN)
    return -1;
  if (!given(b, 6)) return -2;
  const size_t npts = (size_t)W * B;
  Dev D(b, 6);
  SP_NEED(0, cap * NW); SP_NEED(1, npts); SP_NEED(2, npts); SP_NEED(3, W + 1); SP_NEED(4, nhot); SP_NEED(5, nhot * split * NW);
  const uint32_t *cnt = hw(b, 1), *rel = hw(b, 2), *base = hw(b, 3), *hl = hw(b, 4);
  for (uint64_t i = 0; i < nhot; ++i) {
    const uint32_t t = hl[i];
    if (t >= npts || cnt[t] < 1 || (uint64_t)base[t / B] + rel[t] + cnt[t] > cap) return -2;
  }
  const Level L{D.u(1), D.u(2), D.u(3)};
  if (D.ok()) {
    if (which == 0) hipLaunchKernelGGL(k_hot_sum<KF>, dim3((unsigned)nhot, (unsigned)split), dim3(256), 36 * 256 * 4, 0, D.u(0), L, B, D.u(4), D.u(5), (uint32_t)split);
    else hipLaunchKernelGGL(k_hot_fold<KF>, dim3((unsigned)nhot), dim3(256), 36 * 256 * 4, 0, D.u(0), L, B, D.u(4), D.u(5), (uint32_t)split);
  }
  return D.finish();
}

// the resident forms: fmt64 = 0 the limb form (2 * PE words per point), 1 the 64-byte form (2 * PK words per point)
template <class Cfg>
int bases_prep(const KBuf* b, const int64_t* p) {
  using F = typename Cfg::F;
  const size_t n = (size_t)p[1];
  const int fmt64 = (int)p[2];
  if (p[1] < 1 || p[1] > (1 << 22) || (fmt64 != 0 && fmt64 != 1)) return -1;
  if (!b[0].host || !b[2].host) return -2;
  const size_t wpp = fmt64 ? 2 * BaseIO<F>::PK : 2 * BaseIO<F>::PE;
  Dev D(b, 3);
  SP_NEED(0, n * BaseIO<F>::W * 2); SP_NEED(2, n * wpp);
  if (b[1].host && b[1].bytes < n) return -2;
  if (D.ok()) launch_prep_bases<F>(0, D.at<uint64_t>(0), D.at<uint8_t>(1), n, D.u(2), fmt64 != 0);
  return D.finish();
}

template <class Cfg>
int bases_table_next(const KBuf* b, const int64_t* p) {
  using F = typename Cfg::F;
  const size_t n = (size_t)p[1];
  const int c = (int)p[2], fmt64 = (int)p[3];
  if (p[1] < 1 || p[1] > (1 << 22) || c < 1 || c > 20 || (fmt64 != 0 && fmt64 != 1)) return -1;
  if (!given(b, 2)) return -2;
  const size_t wpp = fmt64 ? 2 * BaseIO<F>::PK : 2 * BaseIO<F>::PE;
  Dev D(b, 2);
  SP_NEED(0, n * wpp); SP_NEED(1, n * wpp);
  if (D.ok()) hipLaunchKernelGGL(k_table_next<F>, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, 0, D.u(0), n, c, D.u(1), fmt64);
  return D.finish();
}

// k_acc_tasks<F>.  Every entry every task of the caller's lists reads, and the base it names in every set, is looked up on the host copies
// first (the rules of msm_common.h for a bucket's task length are applied to RANGES only: which entries a task covers).
template <class Cfg>
int acc_tasks(const KBuf* b, const int64_t* p) {
  using F = typename Cfg::F;
  constexpr uint32_t NW = (uint32_t)PointIO<F>::NW;
  const int nsets = (int)p[1], W = (int)p[3], B = (int)p[4], mshift = (int)p[6], top_w = (int)p[8];
  const uint64_t n = (uint64_t)p[2], cap = (uint64_t)p[9];
  const uint32_t T0 = (uint32_t)p[5], T_top = (uint32_t)p[7];
  if (nsets < 1 || nsets > MAX_FUSED || p[2] < 1 || W < 1 || B < 1 || (uint64_t)W * B > ((uint64_t)1 << 20) || n > ((uint64_t)1 << 24) || mshift < 0 || mshift > 24 ||
      top_w >= W || p[9] < 1 || cap * NW * 4 >= SPAN || (mshift && W != 1))
    return -1;
  for (uint32_t T : {T0, T_top})
    if (((T & T_MASK) >> (T >> 30)) < 1) return -1;
  uint64_t idx_off[MAX_FUSED], tab_n[MAX_FUSED], nbases[MAX_FUSED], wpb[MAX_FUSED];
  int fmt[MAX_FUSED];
  for (int k = 0; k < nsets; ++k) {
    idx_off[k] = (uint64_t)p[10 + 4 * k]; tab_n[k] = (uint64_t)p[11 + 4 * k]; fmt[k] = (int)p[12 + 4 * k]; nbases[k] = (uint64_t)p[13 + 4 * k];
    if (p[10 + 4 * k] < 0 || p[11 + 4 * k] < 0 || p[13 + 4 * k] < 1 || nbases[k] > ((uint64_t)1 << 24) || fmt[k] < BASES_72 || fmt[k] > BASES_ABI ||
        (fmt[k] == BASES_ABI && !BaseIO<F>::HAS_ABI))
      return -1;
    wpb[k] = fmt[k] == BASES_ABI ? 16 : fmt[k] == BASES_64 ? 2 * BaseIO<F>::PK : 2 * BaseIO<F>::PE;
    if (!b[8 + k].host || !b[11 + k].host) return -2;
  }
  if (!given(b, 8)) return -2;
  const size_t npts = (size_t)W * B;
  Dev D(b, 14);
  SP_NEED(0, (uint64_t)W * n); SP_NEED(1, npts); SP_NEED(2, npts); SP_NEED(3, npts); SP_NEED(4, npts); SP_NEED(5, W + 1);
  const uint32_t *sorted = hw(b, 0), *bstart = hw(b, 1), *bsize = hw(b, 2), *rel = hw(b, 4), *base = hw(b, 5), *task_bkt = hw(b, 6), *task_id = hw(b, 7);
  const uint64_t ntasks = base[W];
  if (ntasks < 1 || ntasks > cap) return -2;
  SP_NEED(6, ntasks); SP_NEED(7, ntasks);
  for (int k = 0; k < nsets; ++k) { SP_NEED(8 + k, nbases[k] * wpb[k]); SP_NEED(11 + k, cap * NW); }
  for (uint64_t q = 0; q < ntasks; ++q) {
    const uint64_t bi = task_bkt[q], t = task_id[q];
    if (bi >= npts || t >= cap) return -2;
    const int w = (int)(bi / B);
    if (t < (uint64_t)base[w] + rel[bi]) return -2;
    const uint64_t seg = t - base[w] - rel[bi], len_all = bsize[bi];
    const uint32_t Tw = w == top_w ? T_top : T0, tp = Tw & T_MASK;
    const uint64_t T = len_all > (uint64_t)GATHER_SUM_MAX * tp ? tp >> (Tw >> 30) : tp;
    const uint64_t lo = seg * T, hi = lo + T < len_all ? lo + T : len_all;
    if (lo >= len_all || (uint64_t)bstart[bi] + len_all > n) return -2;
    for (uint64_t j = lo; j < hi; ++j) {
      const uint32_t e = sorted[(size_t)w * n + bstart[bi] + j];
      for (int k = 0; k < nsets; ++k) {
        uint64_t idx = e & 0x7fffffffu, row = 0;
        if (mshift) { row = (idx >> mshift) * tab_n[k]; idx &= ((uint64_t)1 << mshift) - 1; }
        if (idx < idx_off[k]) continue;
        if (row + (idx - idx_off[k]) >= nbases[k]) return -2;
      }
    }
  }
  AccSets A;
  A.nsets = nsets;
  for (int k = 0; k < MAX_FUSED; ++k) { A.pb[k] = nullptr; A.idx_off[k] = 0; A.partial[k] = nullptr; A.tab_n[k] = 0; A.fmt[k] = BASES_72; }
  for (int k = 0; k < nsets; ++k) { A.pb[k] = D.u(8 + k); A.idx_off[k] = (uint32_t)idx_off[k]; A.partial[k] = D.u(11 + k); A.tab_n[k] = (uint32_t)tab_n[k]; A.fmt[k] = (uint8_t)fmt[k]; }
  const Level L0{D.u(3), D.u(4), D.u(5)};
  if (D.ok())
    hipLaunchKernelGGL(k_acc_tasks<F>, dim3((unsigned)((ntasks + 63) / 64) * (unsigned)nsets), dim3(64), 0, 0, A, D.u(0), D.u(1), D.u(2), L0, D.u(6), D.u(7), (size_t)n, W, B, T0,
                       (size_t)cap, mshift, T_top, top_w);
  return D.finish();
}

#define RP_CURVE(fn, b, p) ((p)[0] == 0 ? fn<kg::msm::G1Cfg>(b, p) : (p)[0] == 1 ? fn<kg::msm::GkCfg>(b, p) : (p)[0] == 2 ? fn<kg::msm::G2Cfg>(b, p) : -1)

}  // namespace reduceprobe

extern "C" {

// A point of `part` / `pin` / `pout` / `scratch` is PointAoS: NW = 36 words (G2: 72, x.c0 x.c1 y.c0 .. zzz.c1), nine limbs per element.
// A point of `buckets` / `in` / `out` lies in the PointIO structure of arrays: word k of item i at [k * stride + i] (G2: 72 planes, the
// c0 planes of a coordinate before its c1 planes).  Level tables: cnt, rel [W][B], base [W + 1].

// k_prep_bases<F, P64>: the ABI form (x | y, four 64-bit words per base-field element, R = 2^256) -> a resident form
// b: 0 bases (n points), 1 inf (n bytes) or null, 2 out io (n resident points)
// p: 0 curve, 1 n, 2 fmt64 (0: the limb form, INF_BIT in word 8; 1: the 64-byte form, INF_BIT in word 7)
int dp_bases_prep(const reduceprobe::KBuf* b, const int64_t* p) { return RP_CURVE(reduceprobe::bases_prep, b, p); }

// k_table_next<F>: next[i] = 2^c * prev[i], both in the resident form fmt64 names
// b: 0 prev (n resident points), 1 next io
// p: 0 curve, 1 n, 2 c, 3 fmt64
int dp_bases_table_next(const reduceprobe::KBuf* b, const int64_t* p) { return RP_CURVE(reduceprobe::bases_table_next, b, p); }

// k_acc_tasks<F> for nsets = 1 .. 3 base arrays over one sort.  A merged sort (mshift > 0) has W = 1 bucket window, entries that carry
// (window << mshift | scalar), and base arrays that are tables of windows x tab_n rows.
// b: 0 sorted ([W][n]), 1 bstart, 2 bsize, 3 cnt, 4 rel ([W][B]), 5 base (W + 1), 6 task_bkt, 7 task_id (base[W] words), 8 .. 10 the sets' base
//    arrays (fmt 0: limb form, 1: 64-byte form, 2: the caller's ABI array), 11 .. 13 the sets' partial sums io (part_cap PointAoS points)
// p: 0 curve, 1 nsets, 2 n (row length of sorted), 3 W, 4 B, 5 T0, 6 mshift, 7 T_top, 8 top_w, 9 part_cap, then per set: idx_off, tab_n, fmt, points in
//    the base array
int dp_acc_tasks(const reduceprobe::KBuf* b, const int64_t* p) { return RP_CURVE(reduceprobe::acc_tasks, b, p); }

// which 0: k_gather_buckets<F>; 1: k_gather_halve<KF> (B even; out = level 1, stride W * 2 * (B / 2)); 2: k_gather_sum<F, KF>
// b: 0 pin (cap points), 1 cnt, 2 rel, 3 base, 4 out io (W * B points, stride W * B)
// p: 0 curve, 1 which, 2 W, 3 B, 4 cap (points in pin)
int dp_gather(const reduceprobe::KBuf* b, const int64_t* p) { return RP_CURVE(reduceprobe::gather, b, p); }

// k_sum_tasks<KF>: launched over `bound` tasks (the product's bound: the previous round's task count), of which base_out[W] exist
// b: 0 pin (in_cap points), 1 cnt_in, 2 rel_in, 3 base_in, 4 cnt_out, 5 rel_out, 6 base_out, 7 pout io (out_cap points)
// p: 0 curve, 1 W, 2 B, 3 T2, 4 bound, 5 in_cap, 6 out_cap
int dp_sum_tasks(const reduceprobe::KBuf* b, const int64_t* p) { return RP_CURVE(reduceprobe::sum_tasks, b, p); }

// k_halve<KF>: W windows of narr_in arrays of 2 n_out items -> narr_in + 1 arrays of n_out items
// b: 0 in (in_stride items), 1 out io (out_stride items)
// p: 0 curve, 1 W, 2 narr_in, 3 n_out, 4 in_stride, 5 out_stride
int dp_halve(const reduceprobe::KBuf* b, const int64_t* p) { return RP_CURVE(reduceprobe::halve, b, p); }

// form 0: k_reduce_tail<KF, E64, TL> (len = TL); 1: k_reduce_tail<KF, E64, 0> (len <= TL / 2); 2: k_reduce_tail_coop<F, E64> (len <= TL)
// b: 0 in (in_stride items), 1 out io (the exported slot: W * c points of 4 * E64 u64 words, x | y | zz | zzz, R = 2^256)
// p: 0 curve, 1 form, 2 W, 3 narr, 4 len (a power of two), 5 c (>= narr + log2 len), 6 in_stride
int dp_reduce_tail(const reduceprobe::KBuf* b, const int64_t* p) { return RP_CURVE(reduceprobe::reduce_tail, b, p); }

// which 0: k_hot_sum<KF> (scratch io); 1: k_hot_fold<KF> (part io)
// b: 0 part (cap points), 1 cnt, 2 rel, 3 base, 4 hot_list (nhot bucket numbers w * B + b), 5 scratch (nhot * split points)
// p: 0 curve, 1 which, 2 B, 3 nhot, 4 split (<= 256 task lanes, 128 lane pairs), 5 W, 6 cap (points in part)
int dp_hot(const reduceprobe::KBuf* b, const int64_t* p) { return RP_CURVE(reduceprobe::hot, b, p); }

}  // extern "C"
