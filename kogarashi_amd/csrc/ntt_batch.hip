// ntt_batch.hip -- many Fr transforms of one size in one launch per plan step (kg_ntt_bn254_fr_batch, kg_fr_divide_by_z_on_coset_batch).
//
// A transform of up to 2^11 elements is ONE workgroup (ntt.hip: a single row step, ntiles == 1), so a host with B polynomials of one
// size -- the idft -> coset_dft chains of groth16/src/prover.rs:36-41, the columns of a trace -- paid B launches that each used under
// 1 % of the chip.  The tile code (ntt_tile.h) reads blockIdx.x only, so the grid's y dimension carries the transform's index here: the
// kernel below runs k_ntt_tile's body (ntt_tile_run) with `in` and `out` advanced by blockIdx.y times a per-step element stride
// (ntt_batch.h), and every step of the plan is one launch for a whole group of transforms.  Twiddle tables are the context's cached ones
// (ntt_tables), shared by all transforms of the batch.  One body, two kernel shells: k_ntt_tile given the two strides and a grid of
// (tiles, 1) takes 6 VGPRs more in four of its shapes, and two of them lose a wave per SIMD (EXPERIMENTS.md Part S).  This file is a
// translation unit of its own so that its instantiations compile beside ntt.hip's instead of doubling that file's compile time.
#include "common.h"
#include "ntt_core.h"
#include "ntt_tile.h"
#include "ntt_batch.h"

using namespace kg;

static_assert(NTT_BATCH_ONE_STEP_MAX_LOG == (uint32_t)NTT_MAX_LOG_M, "ntt_batch.h: the one-step limit is ntt_plan's");

namespace {

// k_ntt_tile over a group of transforms: workgroup (x, y) runs tile x of transform y.  in_stride / out_stride: elements between two
// transforms in the step's source and destination (one element = 4 words).
template <int LOG_M, int LOG_TC, bool ROW>
__global__ void __launch_bounds__((NttTile<Fr, LOG_M, LOG_TC, ROW>::NT)) __attribute__((amdgpu_waves_per_eu(KG_NTT_WAVES))) k_ntt_tile_batch(NttStepArgs A, size_t in_stride, size_t out_stride) {   // <= 128 VGPRs: LDS admits four waves per SIMD
  KG_SERVICE_PRIO();
  extern __shared__ uint32_t lds[];
  A.in += (size_t)blockIdx.y * in_stride * 4;
  A.out += (size_t)blockIdx.y * out_stride * 4;
  ntt_tile_run<NttTile<Fr, LOG_M, LOG_TC, ROW>>(A, lds);
}

// element i of transform b *= c   (c: one internal-form constant in device memory); workgroups of transform b: blockIdx.y = b
__global__ void __launch_bounds__(256) k_scale_const_batch(uint64_t* __restrict__ data, size_t n, size_t stride, const uint32_t* __restrict__ c) {
  KG_SERVICE_PRIO();
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const size_t e = (size_t)blockIdx.y * stride + i;
  uint32_t w[8];
  load_words(data, e, w);
  Fr v = mul(limbs_from_words<FrParams>(w), NttIO<Fr>::table(c, 0));
  words_from_limbs(reduce_2p(v), w);
  store_words(data, e, w);
}

// ---- dispatch: the shapes launch_step (ntt.hip) dispatches, batched ------------------------------------------------------------
template <int LOG_M, int LOG_TC, bool ROW>
int launch_tile_batch(NttShape<LOG_M, LOG_TC, ROW>, kg_ctx* ctx, hipStream_t st, const NttStepArgs& a, uint32_t ntiles, uint32_t group, NttBatchStrides s) {
  using T = NttTile<Fr, LOG_M, LOG_TC, ROW>;
  if (T::LDS_BYTES > 48 * 1024)            // more than the default dynamic LDS limit needs the attribute on THIS symbol (per device: set at every launch)
    KG_HIP(ctx, hipFuncSetAttribute((const void*)k_ntt_tile_batch<LOG_M, LOG_TC, ROW>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)T::LDS_BYTES));
  hipLaunchKernelGGL((k_ntt_tile_batch<LOG_M, LOG_TC, ROW>), dim3(ntiles, group), dim3(T::NT), T::LDS_BYTES, st, a, s.in, s.out);
  return KG_OK;
}
int launch_step_batch(kg_ctx* ctx, hipStream_t st, const NttStepDesc& d, const NttStepArgs& a, uint32_t ntiles, uint32_t group, NttBatchStrides s) {
  int rc = KG_OK;
  if (!ntt_for_shape(d, [&](auto shape) { rc = launch_tile_batch(shape, ctx, st, a, ntiles, group, s); }))
    return set_err(ctx, KG_ERR_UNSUPPORTED, "ntt tile shape not instantiated");
  return rc;
}

}  // namespace

extern "C" {

int kg_ntt_batch_plan(uint32_t log_n, size_t count, size_t* per_launch) {
  if (per_launch) *per_launch = ntt_batch_per_launch(log_n);
  const size_t g = ntt_batch_groups(log_n, count);
  return g > (size_t)INT_MAX ? INT_MAX : (int)g;
}

int kg_ntt_bn254_fr_batch(kg_ctx* ctx, uint64_t* d_data, uint32_t log_n, size_t count, size_t stride, int inverse, int coset) {
  return kg::kg_guarded(ctx, [&]() -> int {
  if (!ntt_batch_args_ok(ctx, d_data, log_n, count, stride)) return KG_ERR_BAD_ARG;
  if (count == 0) return KG_OK;
  KG_HIP(ctx, hipSetDevice(ctx->device));
  inverse = inverse ? 1 : 0;
  const size_t n = (size_t)1 << log_n;
  NttTables tabs;
  KG_TRY(ntt_tables(ctx, log_n, inverse, &tabs, nullptr));
  NttStepDesc d[3];
  const int nsteps = ntt_plan(log_n, tuning().ntt_steps, d, tuning().ntt_tile);    // the plan the tables were built for (ntt.hip)
  uint64_t* tmp = nullptr;
  if (nsteps > 1) {
    KG_TRY(ctx->ws2.ensure(DevMem{ctx, "ntt buffer allocation"}, ntt_batch_scratch_elems(log_n, count) * 32));
    tmp = ctx->ws2.as<uint64_t>();
  }
  const size_t per = ntt_batch_per_launch(log_n), groups = ntt_batch_groups(log_n, count);
  hipStream_t st = ctx->stream;
  PhaseScope ph(ctx, "ntt_batch", st);
  for (size_t g = 0; g < groups; ++g) {                  // one after another on the stream: every group uses the same scratch
    const NttBatchGroup grp = ntt_batch_group(per, count, g);
    for (int i = 0; i < nsteps; ++i) {
      NttStepArgs a;
      const uint32_t ntiles = ntt_step_args(log_n, nsteps, d, i, tabs, d_data + grp.first * stride * 4, tmp, inverse, coset, a);
      KG_TRY(launch_step_batch(ctx, st, d[i], a, ntiles, (uint32_t)grp.count, ntt_batch_step_strides(nsteps, i, n, stride)));
    }
  }
  ph.end();
  KG_HIP(ctx, hipGetLastError());
  return KG_OK;
  });
}

int kg_fr_divide_by_z_on_coset_batch(kg_ctx* ctx, uint64_t* d_data, uint32_t log_n, size_t count, size_t stride) {
  if (!ntt_batch_args_ok(ctx, d_data, log_n, count, stride)) return KG_ERR_BAD_ARG;
  if (count == 0) return KG_OK;
  KG_HIP(ctx, hipSetDevice(ctx->device));
  NttTables tabs;
  const uint32_t* zinv = nullptr;
  KG_TRY(ntt_tables(ctx, log_n, 0, &tabs, &zinv));
  const size_t n = (size_t)1 << log_n;
  for (size_t first = 0; first < count; first += NTT_BATCH_GRID_Y_MAX) {     // no scratch: the grid's y limit alone cuts the batch
    const size_t cnt = count - first < NTT_BATCH_GRID_Y_MAX ? count - first : NTT_BATCH_GRID_Y_MAX;
    hipLaunchKernelGGL(k_scale_const_batch, dim3((unsigned)((n + 255) / 256), (unsigned)cnt), dim3(256), 0, ctx->stream, d_data + first * stride * 4, n, stride, zinv);
  }
  KG_HIP(ctx, hipGetLastError());
  return KG_OK;
}

}  // extern "C"
