// devprobe_sort.h -- TEST-ONLY entries of libdevprobe.so (included by devprobe.hip) for the integer kernels of the long MSM's scalar side:
// msm_sort_kernels.h, msm_task_kernels.h and msm_level_kernels.h, included unchanged and launched ONE AT A TIME on tables the caller built
// (tests/sort_cases.py: the reference's tables, never the output of an earlier launch).  Nothing here restates product arithmetic.
//
// Every entry has the signature  int dp_xxx(const KBuf* b, const int64_t* p):  b lists HOST arrays, p the scalar parameters (both documented
// at the entry).  A buffer is uploaded whole, and an `io` buffer is copied back whole after the launch -- the caller appends a guard region
// behind the words the kernel owns and fills owned words and guard with patterns of its choice, so the guard travels to the device and
// back with the buffer.  A null host pointer stands for a null device pointer.  The int result is the first HIP status that was not
// hipSuccess (0: ok), -1 for a parameter outside what the kernel is built for, -2 for a buffer shorter than the launch can touch (nothing
// is launched then).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstddef>
#include <vector>
#include "../../kogarashi_amd/csrc/msm_sort_kernels.h"
#include "../../kogarashi_amd/csrc/msm_task_kernels.h"

namespace sortprobe {
using namespace kg;
using namespace kg::msm;

struct KBuf { void* host; uint64_t bytes; uint32_t io; uint32_t reserved; };

struct Dev {
  hipError_t st = hipSuccess;
  const KBuf* b;
  int nb;
  std::vector<void*> d;
  Dev(const KBuf* bufs, int count) : b(bufs), nb(count), d((size_t)count, nullptr) {
    for (int i = 0; i < nb && st == hipSuccess; ++i) {
      if (!b[i].host) continue;
      st = hipMalloc(&d[i], b[i].bytes + 16);
      if (st == hipSuccess && b[i].bytes) st = hipMemcpy(d[i], b[i].host, b[i].bytes, hipMemcpyHostToDevice);
    }
  }
  ~Dev() { for (void* p : d) if (p) (void)hipFree(p); }
  bool ok() const { return st == hipSuccess; }
  void keep(hipError_t e) { if (st == hipSuccess) st = e; }
  template <class T> T* at(int i) const { return reinterpret_cast<T*>(d[i]); }
  uint32_t* u(int i) const { return at<uint32_t>(i); }
  bool words(int i, uint64_t cnt) const { return !b[i].host || b[i].bytes >= cnt * 4; }     // the buffer holds at least cnt 32-bit words
  int finish() {                                      // after the launch: its status, the kernel's, then every io buffer back
    if (st == hipSuccess) st = hipGetLastError();
    if (st == hipSuccess) st = hipDeviceSynchronize();
    for (int i = 0; i < nb && st == hipSuccess; ++i)
      if (b[i].host && b[i].io && b[i].bytes) st = hipMemcpy(b[i].host, d[i], b[i].bytes, hipMemcpyDeviceToHost);
    return (int)st;
  }
};
#define SP_NEED(i, cnt) do { if (!D.words((i), (uint64_t)(cnt))) return -2; } while (0)

inline Words8 words8(const uint32_t* h) { Words8 H; for (int j = 0; j < 8; ++j) H.w[j] = h[j]; return H; }
inline bool window_ok(int c, int W) { return c >= 2 && c <= 20 && W >= 1 && (size_t)W * c <= 256 + (size_t)c; }

// locate_task, one thread per task: out[3 t ..] = window, bucket, segment index
__global__ void __launch_bounds__(256) k_locate(Level L, int W, int B, uint32_t ntasks, uint32_t* out) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= ntasks) return;
  int w, b;
  uint32_t seg;
  locate_task(L, W, B, t, w, b, seg);
  out[3 * (size_t)t] = (uint32_t)w; out[3 * (size_t)t + 1] = (uint32_t)b; out[3 * (size_t)t + 2] = seg;
}

template <class SP>
int prep(Dev& D, const KBuf* b, const int64_t* p) {
  const size_t n = (size_t)p[1];
  const Words8 H = words8((const uint32_t*)b[1].host);
  if (p[2] == 0) {
    hipLaunchKernelGGL(k_prep_scalars<SP>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, D.at<uint64_t>(0), n, H, D.u(2));
    return D.finish();
  }
  const int c = (int)p[3], W = (int)p[4], shift = (int)p[5], G = (int)p[6], nch = (int)p[7], per_wg = (int)p[9];
  const size_t chunk_len = (size_t)p[8];
  if (!window_ok(c, W) || G < 1 || G > 1024 || (per_wg != PREP_CH && per_wg != PREP_CH / 4) || chunk_len == 0 || chunk_len % PREP_CH || nch < 1 ||
      (size_t)nch * chunk_len < n || ((1 << (c - 1)) >> shift) > G)
    return -1;
  SP_NEED(3, (size_t)W * nch * G);
  const size_t hl = (size_t)W * G * 4;
  if (hl > 160 * 1024) return -1;
  if (hl > 48 * 1024) D.keep(hipFuncSetAttribute((const void*)k_prep_scalars_count<SP>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)hl));
  if (D.ok())
    hipLaunchKernelGGL(k_prep_scalars_count<SP>, dim3((unsigned)((n + per_wg - 1) / per_wg)), dim3(PREP_NT), hl, 0, D.at<uint64_t>(0), n, H, D.u(2), c, W, shift, G,
                       nch, chunk_len, D.u(3), per_wg);
  return D.finish();
}

template <int FB>
int group_scatter(Dev& D, const int64_t* p) {
  using E = typename Ent<FB>::T;
  const int tile = (int)p[1], nt = (int)p[2], gridw = (int)p[3], nch = (int)p[4], c = (int)p[6], W = (int)p[7], G = (int)p[9], mshift = (int)p[10], w0 = (int)p[11];
  const size_t n = (size_t)p[5], chunk_len = (size_t)p[8];
  const bool merged = D.b[5].host != nullptr;
  if (!window_ok(c, W) || G < 1 || G > GS_MAXG || ((1 << (c - 1)) >> FB) > G || w0 < 0 || gridw < 1 || w0 + gridw > W || nch < 1 || chunk_len == 0 ||
      (size_t)nch * chunk_len < n || n == 0 || n > ((size_t)1 << 24) || (merged && (mshift < 0 || mshift > 24 || ((size_t)W << mshift) > ((size_t)1 << 24))))
    return -1;
  SP_NEED(0, 8 * n); SP_NEED(1, (size_t)W * nch * G); SP_NEED(2, merged ? (size_t)G : (size_t)W * G); SP_NEED(5, (size_t)W * G);
  SP_NEED(4, (size_t)W * n * (sizeof(E) / 4));
  if (D.ok())
    D.keep(launch_gs_big_any<FB>(tile, nt, dim3(gridw, nch), 0, D.u(0), n, c, W, chunk_len, G, D.u(1), D.u(2), D.at<E>(4), D.u(5), mshift, w0));
  return D.finish();
}

// The caller's tables keep every access of the fine pass inside its rows of n entries: looked at on the HOST copies before anything is
// launched (a table that points outside would be a kernel writing out of bounds).  Not a check of the kernels: only ranges.
template <int FB>
inline bool fine_tables_ok(const KBuf* b, int Wg, size_t n, int G, int B, int maxseg, bool scatter) {
  constexpr uint32_t FINE = 1u << FB, SEGN = SegLen<FB>::V;
  const uint32_t *gstart = (const uint32_t*)b[1].host, *gsize = (const uint32_t*)b[2].host, *segbase = (const uint32_t*)b[3].host;
  const uint32_t *bstart = (const uint32_t*)b[4].host, *segcnt = (const uint32_t*)b[5].host, *segoff = (const uint32_t*)b[6].host;
  for (int w = 0; w < Wg; ++w) {
    const uint32_t* sb = segbase + (size_t)w * (G + 1);
    const uint32_t nseg = sb[G] & ~MULTI_SEG;
    if (nseg > (uint32_t)maxseg || sb[0] != 0) return false;
    for (int g = 0; g < G; ++g) {
      const uint64_t st = gstart[(size_t)w * G + g], sz = gsize[(size_t)w * G + g];
      const uint32_t s0 = sb[g], s1 = g + 1 < G ? sb[g + 1] : nseg;
      if (st + sz > n || s1 < s0 || s1 > nseg || (uint64_t)(s1 - s0) * SEGN < sz) return false;
      if (!scatter || sz <= SEGN) continue;
      for (uint32_t s = s0; s < s1; ++s)
        for (uint32_t f = 0; f < FINE; ++f) {
          const size_t o = ((size_t)w * maxseg + s) * FINE + f;
          if ((uint64_t)bstart[(size_t)w * B + (size_t)g * FINE + f] + segoff[o] + segcnt[o] > n || segcnt[o] > SEGN) return false;
        }
    }
  }
  return true;
}

template <int FB>
int fine_local(Dev& D, const int64_t* p) {
  using E = typename Ent<FB>::T;
  const int Wg = (int)p[1], gridy = (int)p[2], G = (int)p[4], B = (int)p[5], maxseg = (int)p[6];
  const size_t n = (size_t)p[3];
  constexpr uint32_t FINE = 1u << FB;
  if (Wg < 1 || gridy < 1 || gridy > maxseg || G < 1 || G > 1024 || (size_t)B != (size_t)G * FINE) return -1;
  SP_NEED(0, (size_t)Wg * n * (sizeof(E) / 4)); SP_NEED(1, (size_t)Wg * G); SP_NEED(2, (size_t)Wg * G); SP_NEED(3, (size_t)Wg * (G + 1));
  SP_NEED(4, (size_t)Wg * B); SP_NEED(5, (size_t)Wg * maxseg * FINE); SP_NEED(6, (size_t)Wg * maxseg * FINE); SP_NEED(7, (size_t)Wg * n);
  if (!fine_tables_ok<FB>(D.b, Wg, n, G, B, maxseg, false)) return -2;
  D.keep(hipFuncSetAttribute((const void*)k_fine_local<FB>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)fine_local_lds<FB>()));
  if (D.ok())
    hipLaunchKernelGGL(k_fine_local<FB>, dim3(Wg, gridy), dim3(512), fine_local_lds<FB>(), 0, D.at<const E>(0), n, G, B, maxseg, D.u(1), D.u(2), D.u(3), D.u(4), D.u(5),
                       D.u(6), D.u(7));
  return D.finish();
}

template <int FB>
int fine_scatter(Dev& D, const int64_t* p) {
  using E = typename Ent<FB>::T;
  const int gridx = (int)p[1], gridy = (int)p[2], G = (int)p[4], B = (int)p[5], maxseg = (int)p[6], Wg = (int)p[7], extra_w = (int)p[8];
  const size_t n = (size_t)p[3];
  constexpr uint32_t FINE = 1u << FB;
  if (Wg < 1 || gridy < 1 || G < 1 || G > 1024 || (size_t)B != (size_t)G * FINE || gridx < Wg || (gridx > Wg && (extra_w < 0 || extra_w >= Wg)) || extra_w >= Wg) return -1;
  SP_NEED(0, (size_t)Wg * n * (sizeof(E) / 4)); SP_NEED(1, (size_t)Wg * G); SP_NEED(2, (size_t)Wg * G); SP_NEED(3, (size_t)Wg * (G + 1));
  SP_NEED(4, (size_t)Wg * B); SP_NEED(5, (size_t)Wg * maxseg * FINE); SP_NEED(6, (size_t)Wg * maxseg * FINE); SP_NEED(7, (size_t)Wg * n);
  if (!fine_tables_ok<FB>(D.b, Wg, n, G, B, maxseg, true)) return -2;
  D.keep(hipFuncSetAttribute((const void*)k_fine_scatter<FB>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)fine_scatter_lds<FB>()));
  if (D.ok())
    hipLaunchKernelGGL(k_fine_scatter<FB>, dim3(gridx, gridy), dim3(512), fine_scatter_lds<FB>(), 0, D.at<const E>(0), n, G, B, maxseg, D.u(1), D.u(2), D.u(3), D.u(4),
                       D.u(5), D.u(6), D.u(7), Wg, extra_w);
  return D.finish();
}

}  // namespace sortprobe

extern "C" {

using sortprobe::Dev;
using sortprobe::KBuf;

// k_prep_scalars<SP> (p[2] = 0) and k_prep_scalars_count<SP> (p[2] = 1)
// b: 0 scalars (4 n u64), 1 H (8 words, host only), 2 kt io (8 n), 3 cnt io ([W][nch][G], the caller's zeros; count only)
// p: 0 scalar field (0 Fr, 1 Fq), 1 n, 2 count, 3 c, 4 W, 5 shift, 6 G, 7 nch, 8 chunk_len, 9 per_wg
int dp_sort_prep(const KBuf* b, const int64_t* p) {
  if (p[1] < 1 || p[1] >= ((int64_t)1 << 28) || !b[1].host || b[1].bytes < 32) return -1;
  Dev D(b, 4);
  SP_NEED(0, 8 * p[1]); SP_NEED(2, 8 * p[1]);
  return p[0] == 0 ? sortprobe::prep<kg::FrParams>(D, b, p) : sortprobe::prep<kg::FqParams>(D, b, p);
}

// k_count / k_scan_chunks / k_scatter of the one-pass sort (shift = 0) -- p[0] picks the kernel: 0 count, 1 scan, 2 scatter
// b: 0 kt (8 n), 1 cnt ([W][nch][B]; io for count and scan), 2 bsize io ([W][B]; scan), 3 bstart ([W][B]; scatter), 4 sorted io ([W][n]; scatter)
// p: 0 kernel, 1 n, 2 c, 3 W, 4 chunk_len, 5 nch
int dp_sort_onepass(const KBuf* b, const int64_t* p) {
  using namespace sortprobe;
  const int which = (int)p[0], c = (int)p[2], W = (int)p[3], nch = (int)p[5];
  const size_t n = (size_t)p[1], chunk_len = (size_t)p[4];
  if (which < 0 || which > 2 || !window_ok(c, W) || c > 16 || nch < 1 || chunk_len == 0 || (size_t)nch * chunk_len < n || n == 0) return -1;
  const int B = 1 << (c - 1);
  const size_t lds = (size_t)B * 4;
  Dev D(b, 5);
  SP_NEED(0, 8 * n); SP_NEED(1, (size_t)W * nch * B); SP_NEED(2, (size_t)W * B); SP_NEED(3, (size_t)W * B); SP_NEED(4, (size_t)W * n);
  if (which == 0) {
    if (lds > 48 * 1024) D.keep(hipFuncSetAttribute((const void*)k_count, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    if (D.ok()) hipLaunchKernelGGL(k_count, dim3(W, nch), dim3(1024), lds, 0, D.u(0), n, c, W, chunk_len, 0, D.u(1));
  } else if (which == 1) {
    hipLaunchKernelGGL(k_scan_chunks, dim3((unsigned)(((size_t)W * B + 255) / 256)), dim3(256), 0, 0, D.u(1), W, nch, B, D.u(2));
  } else {
    if (lds > 48 * 1024) D.keep(hipFuncSetAttribute((const void*)k_scatter, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    if (D.ok()) hipLaunchKernelGGL(k_scatter, dim3(W, nch), dim3(1024), lds, 0, D.u(0), n, c, W, chunk_len, 0, D.u(1), D.u(3), D.u(4));
  }
  return D.finish();
}

// k_zero through zero_fill: clears p[1] bytes (rounded up to 16, as the product's carved regions allow) from byte offset p[0] of the buffer
// b: 0 buf io
int dp_sort_zero_fill(const KBuf* b, const int64_t* p) {
  if (p[0] < 0 || p[1] < 0 || (p[0] & 15) || (uint64_t)p[0] + (((uint64_t)p[1] + 15) & ~(uint64_t)15) > b[0].bytes) return -2;
  Dev D(b, 1);
  if (D.ok()) sortprobe::zero_fill(0, D.at<char>(0) + p[0], (size_t)p[1]);
  return D.finish();
}

// k_group_scan: p[0] windows (workgroups) of nt threads
// b: 0 cnt io ([W][nch][G]), 1 gsize io ([W][G]), 2 gstart io ([W][G]), 3 segbase io ([W][G + 1]), 4 bsize io ([W][B]), 5 zero io (zwords)
// p: 0 W, 1 nch, 2 G, 3 B, 4 zwords, 5 seg, 6 nt
int dp_sort_group_scan(const KBuf* b, const int64_t* p) {
  using namespace sortprobe;
  const int W = (int)p[0], nch = (int)p[1], G = (int)p[2], B = (int)p[3], zwords = (int)p[4], nt = (int)p[6];
  if (W < 1 || nch < 1 || G < 1 || G > 4 * nt || (nt != 256 && nt != 512) || B < 4 || (B & 3) || zwords < 0 || p[5] < 1) return -1;
  Dev D(b, 6);
  SP_NEED(0, (size_t)W * nch * G); SP_NEED(1, (size_t)W * G); SP_NEED(2, (size_t)W * G); SP_NEED(3, (size_t)W * (G + 1)); SP_NEED(4, (size_t)W * B); SP_NEED(5, zwords);
  if (D.ok()) hipLaunchKernelGGL(k_group_scan, dim3(W), dim3(nt), 0, 0, D.u(0), nch, G, B, D.u(1), D.u(2), D.u(3), D.u(4), D.u(5), zwords, (uint32_t)p[5]);
  return D.finish();
}

// k_merge_groups
// b: 0 gsize ([W][G]), 1 woff io ([W][G]), 2 gsize_m io (G), 3 gstart_m io (G), 4 segbase_m io (G + 1)
// p: 0 W, 1 G
int dp_sort_merge_groups(const KBuf* b, const int64_t* p) {
  using namespace sortprobe;
  const int W = (int)p[0], G = (int)p[1];
  if (W < 1 || G < 1 || G > 4 * GS_NT) return -1;
  Dev D(b, 5);
  SP_NEED(0, (size_t)W * G); SP_NEED(1, (size_t)W * G); SP_NEED(2, G); SP_NEED(3, G); SP_NEED(4, G + 1);
  if (D.ok()) hipLaunchKernelGGL(k_merge_groups, dim3(1), dim3(GS_NT), 0, 0, D.u(0), W, G, D.u(1), D.u(2), D.u(3), D.u(4));
  return D.finish();
}

// k_group_scatter_big<FB, TILE, NT> through launch_gs_big_any; a merged sort iff woff is given
// b: 0 kt (8 n), 1 cnt ([W][nch][G] prefixes), 2 gstart ([W][G], merged: [G]), 3 unused, 4 tmp io ([W][n] entries of 4 or 8 bytes), 5 woff ([W][G]) or null
// p: 0 FB, 1 tile, 2 nt, 3 grid windows, 4 nch, 5 n, 6 c, 7 W, 8 chunk_len, 9 G, 10 mshift, 11 w0
int dp_sort_group_scatter_big(const KBuf* b, const int64_t* p) {
  if (p[0] != 7 && p[0] != 9) return -1;
  Dev D(b, 6);
  return p[0] == 7 ? sortprobe::group_scatter<7>(D, p) : sortprobe::group_scatter<9>(D, p);
}

// k_fine_local<FB>: grid (Wg, gridy)
// b: 0 tmp ([Wg][n] entries), 1 gstart, 2 gsize ([Wg][G]), 3 segbase ([Wg][G + 1]), 4 bsize io ([Wg][B]), 5 segcnt io, 6 segoff io ([Wg][maxseg][FINE]), 7 sorted io ([Wg][n])
// p: 0 FB, 1 Wg, 2 gridy, 3 n, 4 G, 5 B, 6 maxseg
int dp_sort_fine_local(const KBuf* b, const int64_t* p) {
  if (p[0] != 7 && p[0] != 9) return -1;
  Dev D(b, 8);
  return p[0] == 7 ? sortprobe::fine_local<7>(D, p) : sortprobe::fine_local<9>(D, p);
}

// k_fine_scatter<FB>: grid (gridx, gridy), gridx = Wg or Wg + 3
// b: 0 tmp, 1 gstart, 2 gsize, 3 segbase, 4 bstart ([Wg][B]), 5 segcnt, 6 segoff, 7 sorted io
// p: 0 FB, 1 gridx, 2 gridy, 3 n, 4 G, 5 B, 6 maxseg, 7 Wg, 8 extra_w
int dp_sort_fine_scatter(const KBuf* b, const int64_t* p) {
  if (p[0] != 7 && p[0] != 9) return -1;
  Dev D(b, 8);
  return p[0] == 7 ? sortprobe::fine_scatter<7>(D, p) : sortprobe::fine_scatter<9>(D, p);
}

// k_bucket_rows (nsplit = 0), or k_bucket_part followed by k_bucket_fill (nsplit = B / 4096 >= 2)
// b: 0 bsize ([Wg][B]), 1 bstart io, 2 ntask io, 3 rel io ([Wg][B]), 4 row_total io (Wg), 5 maxv io (3 words, the caller's zeros), 6 ghist io (256, zeros),
//    7 hot_list io (hot_cap), 8 part io ([Wg][nsplit][2]; parts only)
// p: 0 Wg, 1 B, 2 T0, 3 T_top, 4 top_w, 5 hot_cap, 6 nsplit
int dp_task_bucket_tables(const KBuf* b, const int64_t* p) {
  using namespace sortprobe;
  const int Wg = (int)p[0], B = (int)p[1], top_w = (int)p[4], nsplit = (int)p[6];
  const uint32_t T0 = (uint32_t)p[2], T_top = (uint32_t)p[3], hot_cap = (uint32_t)p[5];
  if (Wg < 1 || B < 1 || ((T0 & T_MASK) >> (T0 >> 30)) < 1 || ((T_top & T_MASK) >> (T_top >> 30)) < 1 || top_w >= Wg) return -1;
  if (nsplit && (nsplit < 1 || B % nsplit || (B / nsplit) % (4 * BR_NT))) return -1;
  // one workgroup per row: a row whose lanes own whole 16-byte groups is read in vectors, so its start must be 16-byte aligned
  if (!nsplit && (B > 4096 || ((((B + BR_NT - 1) / BR_NT) & 3) == 0 && (B & 3)))) return -1;
  Dev D(b, 9);
  for (int i = 0; i < 4; ++i) SP_NEED(i, (size_t)Wg * B);
  SP_NEED(4, Wg); SP_NEED(5, 3); SP_NEED(6, LEN_BINS); SP_NEED(7, hot_cap); SP_NEED(8, (size_t)Wg * nsplit * 2);
  if (D.ok()) {
    if (nsplit) {
      hipLaunchKernelGGL(k_bucket_part, dim3(Wg, nsplit), dim3(BR_NT), 0, 0, D.u(0), B, T0, nsplit, D.u(8), D.u(5), D.u(6), T_top, top_w, D.u(7), hot_cap);
      hipLaunchKernelGGL(k_bucket_fill, dim3(Wg, nsplit), dim3(BR_NT), 0, 0, D.u(0), B, T0, nsplit, D.u(8), D.u(1), D.u(2), D.u(3), D.u(4), T_top, top_w);
    } else
      hipLaunchKernelGGL(k_bucket_rows, dim3(Wg), dim3(BR_NT), 0, 0, D.u(0), B, T0, D.u(1), D.u(2), D.u(3), D.u(4), D.u(5), D.u(6), T_top, top_w, D.u(7), hot_cap);
  }
  return D.finish();
}

// k_task_bases
// b: 0 row_total (W), 1 base io (W + 1), 2 maxv (3), 3 info io (2), 4 ghist (256), 5 cursor io (256), 6 host_info io (4)
// p: 0 W
int dp_task_bases(const KBuf* b, const int64_t* p) {
  using namespace sortprobe;
  const int W = (int)p[0];
  if (W < 1) return -1;
  Dev D(b, 7);
  SP_NEED(0, W); SP_NEED(1, W + 1); SP_NEED(2, 3); SP_NEED(3, 2); SP_NEED(4, LEN_BINS); SP_NEED(5, LEN_BINS); SP_NEED(6, 4);
  if (D.ok()) hipLaunchKernelGGL(k_task_bases, dim3(1), dim3(64), 0, 0, D.u(0), W, D.u(1), D.u(2), D.u(3), D.u(4), D.u(5), D.u(6));
  return D.finish();
}

// k_len_scatter over total = Wg * B buckets
// b: 0 bsize, 1 ntask, 2 rel ([Wg][B]), 3 base (Wg + 1), 4 cursor io (256: the descending-key starts), 5 task_bkt io, 6 task_id io (cap words each)
// p: 0 Wg, 1 B, 2 T0, 3 T_top, 4 top_w, 5 ntasks (what the tables add up to: the launch is refused if the lists are shorter)
int dp_task_len_scatter(const KBuf* b, const int64_t* p) {
  using namespace sortprobe;
  const int Wg = (int)p[0], B = (int)p[1], top_w = (int)p[4];
  if (Wg < 1 || B < 1 || top_w >= Wg || p[5] < 0) return -1;
  const size_t total = (size_t)Wg * B;
  Dev D(b, 7);
  for (int i = 0; i < 3; ++i) SP_NEED(i, total);
  SP_NEED(3, Wg + 1); SP_NEED(4, LEN_BINS); SP_NEED(5, p[5]); SP_NEED(6, p[5]);
  if (D.ok())
    hipLaunchKernelGGL(k_len_scatter, dim3((unsigned)((total + 1023) / 1024)), dim3(1024), 0, 0, D.u(0), D.u(1), D.u(2), D.u(3), total, B, (uint32_t)p[2], D.u(4), D.u(5),
                       D.u(6), (uint32_t)p[3], top_w);
  return D.finish();
}

// the bookkeeping of a further round (msm_level_kernels.h) -- p[0] picks the kernel: 0 k_task_count, 1 k_scan_rows, 2 k_row_bases, 3 locate_task
// count:  b 0 in (total), 1 ntask io (total), 2 maxv io (1)            p 1 total, 2 T
// scan:   b 0 in ([W][B]), 1 rel io ([W][B]), 2 row_total io (W)        p 1 W, 2 B, 3 threads per workgroup
// bases:  b 0 row_total (W), 1 base io (W + 1), 2 maxv (1) or null, 3 info io (2)     p 1 W
// locate: b 0 base (W + 1), 1 rel ([W][B]), 2 out io (3 ntasks)         p 1 W, 2 B, 3 ntasks
int dp_level_ops(const KBuf* b, const int64_t* p) {
  using namespace sortprobe;
  const int which = (int)p[0];
  if (which < 0 || which > 3 || p[1] < 1) return -1;
  Dev D(b, 4);
  if (which == 0) {
    const size_t total = (size_t)p[1];
    if (p[2] < 1) return -1;
    SP_NEED(0, total); SP_NEED(1, total); SP_NEED(2, 1);
    if (D.ok()) hipLaunchKernelGGL(k_task_count, dim3((unsigned)((total + 1023) / 1024)), dim3(1024), 0, 0, D.u(0), total, (uint32_t)p[2], D.u(1), D.u(2));
  } else if (which == 1) {
    const int W = (int)p[1], B = (int)p[2], nt = (int)p[3];
    if (B < 1 || nt < 64 || nt > 1024 || (nt & 63)) return -1;
    if ((((B + nt - 1) / nt) & 3) == 0 && (B & 3)) return -1;      // rows read in 16-byte vectors must start 16-byte aligned
    SP_NEED(0, (size_t)W * B); SP_NEED(1, (size_t)W * B); SP_NEED(2, W);
    if (D.ok()) hipLaunchKernelGGL(k_scan_rows, dim3(W), dim3(nt), 0, 0, D.u(0), B, D.u(1), D.u(2));
  } else if (which == 2) {
    const int W = (int)p[1];
    SP_NEED(0, W); SP_NEED(1, W + 1); SP_NEED(2, 1); SP_NEED(3, 2);
    if (D.ok()) hipLaunchKernelGGL(k_row_bases, dim3(1), dim3(64), 0, 0, D.u(0), W, D.u(1), D.u(2), D.u(3));
  } else {
    const int W = (int)p[1], B = (int)p[2];
    if (B < 1 || p[3] < 1 || p[3] > ((int64_t)1 << 24)) return -1;
    SP_NEED(0, W + 1); SP_NEED(1, (size_t)W * B); SP_NEED(2, 3 * (size_t)p[3]);
    const Level L{nullptr, D.u(1), D.u(0)};
    if (D.ok()) hipLaunchKernelGGL(k_locate, dim3((unsigned)((p[3] + 255) / 256)), dim3(256), 0, 0, L, W, B, (uint32_t)p[3], D.u(2));
  }
  return D.finish();
}

}  // extern "C"
