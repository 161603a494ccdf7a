// msm_small_batch.hip -- many short MSMs of one length against ONE base array in one call (kg_commit_batch): the commitments of several
// vectors against one key (nova/src/pedersen.rs:15-20 per fold), the public-input sums of many proofs against one vk.ic.
//
// One short MSM is 64 .. 160 workgroups that each wait on a chain of dependent LDS levels (msm_small_kernels.h), then a host chain of
// 127 or 255 doublings per result: a caller with B vectors paid B launches that left most of the chip idle and B host chains.  The
// kernels read blockIdx.x / blockIdx.y only (k_msm_small) and blockIdx.x only (k_msm_small_combine), so the shells below carry the
// vector's index in the next grid dimension and advance three things per vector: the scalars by the caller's stride, the window sums'
// destination and the planes of split windows by one vector's share of the context's batch scratch (msm_small_batch.h).  One body, two
// kernel shells, as for the batched transform (ntt_batch.hip): the single call's kernels keep their argument list and their registers
// (EXPERIMENTS.md Part T).  The window sums never leave the device: k_small_finish_batch runs the host's chain (msm_small_finish.h) with
// one lane per vector, inverts, and writes affine ABI words and flags in stream order.
// Not batched: the KT form (scalars converted once by k_small_prep, from 2049 pairs), its spill space -- the entry runs kg_commit per
// vector there.
#include "msm_small_kernels.h"
#include "msm_small_batch.h"
#include "msm_small_finish.h"
#include <climits>
#include <vector>

using namespace kg;
using namespace kg::msm;

static_assert(MSM_BATCH_PLANES == SM_MAX_R + 1, "msm_small_batch.h: plane points per workgroup are msm_small_kernels.h's");

namespace {

// what a vector adds to the pointers of SmallArgs: u64 words of scalars and window sums, u32 words of planes
struct SmallBatchStrides { size_t scalars, out, planes; };
struct SmallBatchArgs { SmallArgs a; SmallBatchStrides s; };

// The batch's shells around k_msm_small / k_msm_small_combine (msm_small_kernels.h: SmOne is the single call's): the vector is the grid's
// next free dimension -- z for the main kernel, whose grid is (window, bucket range), y for the combine kernel, whose grid is the windows.
template <int DIM>
struct SmVector {
  using Args = SmallBatchArgs;
  static __device__ __forceinline__ SmallArgs of(const SmallBatchArgs& av) {
    const size_t b = DIM == 2 ? blockIdx.z : blockIdx.y;
    SmallArgs a = av.a;
    a.scalars += b * av.s.scalars;
    a.out += b * av.s.out;
    a.planes += b * av.s.planes;              // (not read by an unsplit window)
    return a;
  }
};
template <class F, class SP> constexpr auto k_msm_small_batch = k_msm_small<F, SP, false, SmVector<2>>;
template <class F> constexpr auto k_msm_small_combine_batch = k_msm_small_combine<F, SmVector<1>>;

// One lane per vector: the W window sums of vector i (ABI words, 4 coordinates each) -> its affine point and flag.  W == 0 (empty
// vectors): every point is the identity.
constexpr int FIN_NT = 64;
template <class F>
__global__ void __launch_bounds__(FIN_NT) k_small_finish_batch(const uint64_t* __restrict__ sums, int W, int c, size_t count, uint64_t* __restrict__ out_xy,
                                                               uint8_t* __restrict__ out_inf) {
  constexpr int E = SmIO<F>::E64;
  const size_t i = (size_t)blockIdx.x * FIN_NT + threadIdx.x;
  if (i >= count) return;
  const uint64_t* mine = sums + i * (size_t)W * 4 * E;
  Affine<F> p;
  const bool finite = small_finish_affine<F>(W, c, [mine](int w) {
    const uint64_t* s = mine + (size_t)w * 4 * E;
    return XYZZ<F>{RefIO<F>::load(s), RefIO<F>::load(s + E), RefIO<F>::load(s + 2 * E), RefIO<F>::load(s + 3 * E)};
  }, p);
  uint64_t* dst = out_xy + i * 2 * E;
  if (finite) put_affine_abi(p, dst, out_inf + i);
  else put_identity_abi<F>(dst, out_inf + i);
}

// one launch group: `group` vectors whose scalars begin at a.scalars; window sums and planes in the batch scratch `ws`
template <class F, class SP>
int batch_group(kg_ctx* ctx, hipStream_t st, SmallArgs a, const MsmBatchShape& sh, size_t stride, size_t group, char* ws, uint64_t* d_out_xy, uint8_t* d_out_inf) {
  const int W = msm_batch_windows(sh), NB = msm_batch_ranges(sh);
  uint64_t* sums = (uint64_t*)ws;
  if (W > 0) {
    KG_TRY((lds_attr_once<k_msm_small_batch<F, SP>, k_msm_small_combine_batch<F>>(ctx, 160 * 1024)));      // the whole 160 KiB of LDS for the two shells
    a.out = sums;
    a.planes = NB > 1 ? (uint32_t*)(ws + group * msm_batch_sums_bytes(sh)) : nullptr;
    const SmallBatchArgs av{a, {stride * 4, msm_batch_sums_bytes(sh) / 8, msm_batch_planes_bytes(sh) / 4}};
    PhaseScope ph(ctx, "small_msm_batch", st);
    hipLaunchKernelGGL((k_msm_small_batch<F, SP>), dim3((unsigned)W, (unsigned)NB, (unsigned)group), dim3(SM_NT), small_lds_bytes<F>(a.n, sh.r, false), st, av);
    ph.end();
    if (NB > 1) {
      PhaseScope pc(ctx, "small_combine_batch", st);
      hipLaunchKernelGGL((k_msm_small_combine_batch<F>), dim3((unsigned)W, (unsigned)group), dim3(SM_NT), small_combine_lds_bytes<F>(sh.c, NB), st, av);
      pc.end();
    }
  }
  PhaseScope pf(ctx, "small_finish_batch", st);
  hipLaunchKernelGGL((k_small_finish_batch<F>), dim3((unsigned)((group + FIN_NT - 1) / FIN_NT)), dim3(FIN_NT), 0, st, sums, W, sh.c, group, d_out_xy, d_out_inf);
  pf.end();
  KG_HIP(ctx, hipGetLastError());
  return KG_OK;
}

// Does the batched path take n-pair vectors (of this context, or -- ctx == nullptr -- by the process's settings), and in which shape?  The
// lengths whose blocking call runs the short kernel with workgroups that convert the scalars themselves; n == 0: the finish kernel alone.
bool batch_shape(const kg_ctx* ctx, int curve, size_t n, MsmBatchShape* sh) {
  *sh = MsmBatchShape{curve, 0, 0, false, n};
  if (n == 0) return true;
  int c = 0, r = 0;
  if (!msm_small_plan(ctx, curve, n, &c, &r) || msm_small_kt(ctx, n)) return false;
  sh->c = c; sh->r = r; sh->glv = msm_small_glv(ctx, curve, n);
  return true;
}

// outside the batched kernels' lengths: one blocking kg_commit per vector, the points and flags copied to the device behind them
int batch_fallback(kg_ctx* ctx, int curve, const uint64_t* d_bases, const uint8_t* d_inf, const uint64_t* d_scalars, size_t n, size_t count, size_t stride,
                   uint64_t* d_out_xy, uint8_t* d_out_inf) {
  const size_t pw = affine_words64(curve);
  std::vector<uint64_t> xy(count * pw);
  std::vector<uint8_t> inf(count);
  for (size_t b = 0; b < count; ++b) KG_TRY(kg_commit(ctx, curve, d_bases, d_inf, d_scalars + b * stride * 4, n, xy.data() + b * pw, inf.data() + b));
  KG_HIP(ctx, hipSetDevice(ctx->device));
  KG_HIP(ctx, hipMemcpyAsync(d_out_xy, xy.data(), count * pw * 8, hipMemcpyHostToDevice, ctx->stream));
  KG_HIP(ctx, hipMemcpyAsync(d_out_inf, inf.data(), count, hipMemcpyHostToDevice, ctx->stream));
  KG_HIP(ctx, hipStreamSynchronize(ctx->stream));              // the host arrays end with this call
  return KG_OK;
}

}  // namespace

extern "C" {

int kg_commit_batch_plan(int curve, size_t n, size_t count, size_t* per_launch) {
  if (per_launch) *per_launch = 0;
  MsmBatchShape sh;
  if (!curve_ok(curve) || count == 0 || !batch_shape(nullptr, curve, n, &sh)) return 0;
  const size_t per = msm_batch_per_launch(msm_batch_vector_bytes(sh)), g = msm_batch_groups(per, count);
  if (per_launch) *per_launch = per;
  return g > (size_t)INT_MAX ? INT_MAX : (int)g;
}

int kg_commit_batch(kg_ctx* ctx, int curve, const uint64_t* d_bases, const uint8_t* d_inf, const uint64_t* d_scalars, size_t n, size_t count, size_t stride,
                    uint64_t* d_out_xy, uint8_t* d_out_inf) {
  return kg::kg_guarded(ctx, [&]() -> int {
  if (!msm_batch_args_ok(ctx, curve, d_bases, d_scalars, n, count, stride, d_out_xy, d_out_inf)) return KG_ERR_BAD_ARG;
  if (count == 0) return KG_OK;
  MsmBatchShape sh;
  if (!batch_shape(ctx, curve, n, &sh)) return batch_fallback(ctx, curve, d_bases, d_inf, d_scalars, n, count, stride, d_out_xy, d_out_inf);
  KG_HIP(ctx, hipSetDevice(ctx->device));
  const size_t vb = msm_batch_vector_bytes(sh), per = msm_batch_per_launch(vb), groups = msm_batch_groups(per, count);
  KG_TRY(ctx->ws_small_batch.ensure(DevMem{ctx, "batched short-input scratch"}, msm_batch_scratch_bytes(vb, count)));
  SmallArgs a = small_args(d_bases, d_inf, d_scalars, n, sh.glv, sh.c, sh.r, msm_batch_windows(sh), msm_batch_ranges(sh));      // out, planes: per group (batch_group)
  const size_t pw = affine_words64(curve);
  hipStream_t st = ctx->stream;
  for (size_t g = 0; g < groups; ++g) {                    // one after another on the stream: every group uses the same scratch
    const MsmBatchGroup grp = msm_batch_group(per, count, g);
    a.scalars = d_scalars + grp.first * stride * 4;
    uint64_t* oxy = d_out_xy + grp.first * pw;
    uint8_t* oinf = d_out_inf + grp.first;
    char* ws = ctx->ws_small_batch.as<char>();
    KG_TRY(with_curve(curve, [&](auto cfg) {
      using D = CurveDev<decltype(cfg)>;
      return batch_group<typename D::F, typename D::SP>(ctx, st, a, sh, stride, grp.count, ws, oxy, oinf);
    }));
  }
  return KG_OK;
  });
}

}  // extern "C"
