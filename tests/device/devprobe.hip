// devprobe.hip -- TEST-ONLY device library (tests/device/libdevprobe.so, built by kogarashi_amd/build.py --devprobe with the product's flags).
// Each entry runs one primitive of the product's headers per thread on the GPU: the cases are the host/device templates of
// tests/host/arith_cases.h, the lines tests/host/hosttest.cpp runs on the CPU, so the two outputs can be compared bit for bit.  The entries
// take HOST arrays: allocate, copy in, launch, synchronise, copy out, free; the int result is the first HIP status that was not hipSuccess (0: ok).
// Nothing here restates product arithmetic; the product headers are included unchanged.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstddef>
#include <vector>
#include "../host/arith_cases.h"
#include "../../kogarashi_amd/csrc/msm_small_kernels.h"
#include "../../kogarashi_amd/csrc/msm_reduce_kernels.h"

using namespace kgcase;

namespace {

constexpr int NT = 64;                       // one wave per workgroup

// device copies of host arrays; the first failing status sticks and turns every later step into a no-op
struct Bufs {
  hipError_t st = hipSuccess;
  std::vector<void*> ptrs;
  ~Bufs() { for (void* p : ptrs) (void)hipFree(p); }
  template <class T> T* alloc(size_t cnt) {
    void* d = nullptr;
    if (st != hipSuccess) return nullptr;
    st = hipMalloc(&d, cnt * sizeof(T) + 16);
    if (st != hipSuccess) return nullptr;
    ptrs.push_back(d);
    return (T*)d;
  }
  template <class T> T* in(const T* h, size_t cnt) {
    T* d = alloc<T>(cnt);
    if (st == hipSuccess) st = hipMemcpy(d, h, cnt * sizeof(T), hipMemcpyHostToDevice);
    return d;
  }
  template <class T> T* out(size_t cnt) {
    T* d = alloc<T>(cnt);
    if (st == hipSuccess) st = hipMemset(d, 0, cnt * sizeof(T));
    return d;
  }
  bool ok() const { return st == hipSuccess; }
  void launched() {                          // after a launch: its status, then the kernel's
    if (st == hipSuccess) st = hipGetLastError();
    if (st == hipSuccess) st = hipDeviceSynchronize();
  }
  template <class T> void back(T* h, const T* d, size_t cnt) {
    if (st == hipSuccess) st = hipMemcpy(h, d, cnt * sizeof(T), hipMemcpyDeviceToHost);
  }
};
inline unsigned blocks(size_t n) { return (unsigned)((n + NT - 1) / NT); }

template <class F>
__global__ void __launch_bounds__(NT) k_raw(int op, const uint32_t* a, const uint32_t* b, const uint32_t* c, const uint32_t* d, const uint32_t* k,
                                            uint32_t* out, size_t n) {
  const size_t i = (size_t)blockIdx.x * NT + threadIdx.x;
  if (i >= n) return;
  raw_case<F>(op, a + 9 * i, b + 9 * i, c + 9 * i, d + 9 * i, k + 18 * i, nullptr, out + RAW_OUT * i);
}
template <class G>
__global__ void __launch_bounds__(NT) k_raw2(int op, const uint32_t* a, const uint32_t* b, const uint32_t* c, const uint32_t* d, uint32_t* out, size_t n) {
  const size_t i = (size_t)blockIdx.x * NT + threadIdx.x;
  if (i >= n) return;
  raw2_case<G>(op, a + 18 * i, b + 18 * i, c + 18 * i, d + 18 * i, nullptr, out + RAW_OUT * i);
}
template <class F>
__global__ void __launch_bounds__(NT) k_field(int op, const uint32_t* a, const uint32_t* b, uint32_t* o, size_t n) {
  const size_t i = (size_t)blockIdx.x * NT + threadIdx.x;
  if (i >= n) return;
  constexpr int W = Conv<F>::W;
  field_case<F>(op, a + W * i, b + W * i, o + W * i);
}
template <class F>
__global__ void __launch_bounds__(NT) k_curve(int op, const uint32_t* p, const uint32_t* q, uint32_t* o, uint8_t* inf, size_t n) {
  const size_t i = (size_t)blockIdx.x * NT + threadIdx.x;
  if (i >= n) return;
  constexpr int W = Conv<F>::W;
  inf[i] = (uint8_t)curve_case<F>(op, p + 4 * W * i, q + 4 * W * i, o + 2 * W * i);
}
__global__ void __launch_bounds__(NT) k_small_digits(const uint32_t* k, size_t n, int c, int32_t* digits) {
  const size_t i = (size_t)blockIdx.x * NT + threadIdx.x;
  if (i >= n) return;
  small_digits_case(k + 8 * i, c, digits + 128 * i);
}
template <class L>
__global__ void __launch_bounds__(NT) k_glv_decompose(const uint32_t* k, size_t n, uint32_t* k1, uint32_t* k2, uint8_t* neg) {
  const size_t i = (size_t)blockIdx.x * NT + threadIdx.x;
  if (i >= n) return;
  glv_decompose_case<L>(k + 8 * i, k1 + 4 * i, k2 + 4 * i, neg + 2 * i);
}
template <class L>
__global__ void __launch_bounds__(NT) k_glv_digits(const uint32_t* k, size_t n, int c, int32_t* digits) {
  const size_t i = (size_t)blockIdx.x * NT + threadIdx.x;
  if (i >= n) return;
  glv_digits_case<L>(k + 8 * i, c, digits + 128 * i);
}
// the endomorphism of the short-input MSM (msm_small_kernels.h) on one affine point in the ABI form
template <class F, class SP>
__global__ void __launch_bounds__(NT) k_endo(const uint32_t* pts, uint32_t* o, size_t n) {
  const size_t i = (size_t)blockIdx.x * NT + threadIdx.x;
  if (i >= n) return;
  constexpr int W = Conv<F>::W;
  Affine<F> pt{Conv<F>::in(pts + 2 * W * i), Conv<F>::in(pts + 2 * W * i + W)};
  kg::msm::SmEndo<F, SP>::apply(pt);
  Conv<F>::out(pt.x, o + 2 * W * i);
  Conv<F>::out(pt.y, o + 2 * W * i + W);
}

// coop_add_level then coop_dbl_level over an LDS image: ONE WAVE per workgroup (64 threads, 16 quads), workgroup g works on items
// [g * COOP_ITEMS, (g + 1) * COOP_ITEMS) (X | Y | ZZ | ZZZ in the ABI form) with the per-quad parameters params[(g * 16 + t) * 5 ..]; every item of
// the image goes out through to_affine.  A parameter row that points outside the image makes its quad idle (the host checks them first).
template <class F>
__global__ void __launch_bounds__(NT) k_coop(const uint32_t* items, const uint32_t* params, uint32_t* o, uint8_t* inf, size_t nwg) {
  constexpr int W = Conv<F>::W;
  constexpr uint32_t E = kg::CoopEl<F>::E;
  __shared__ uint32_t img[4 * E * COOP_ITEMS];
  const size_t g = blockIdx.x;
  if (g >= nwg) return;                                  // (uniform over the workgroup: nobody is left waiting at a barrier)
  const uint32_t tid = threadIdx.x;
  const kg::CoopQuad<F> io{img, COOP_ITEMS, nullptr, NT / 4, tid >> 2, nullptr, 0, 0, 0, (int)(tid & 3u)};
  if (tid < COOP_ITEMS) kg::coop_set_point(io, tid, xyzz_in<F>(items + (g * COOP_ITEMS + tid) * 4 * W));
  __syncthreads();
  const uint32_t* pr = params + (g * COOP_QUADS + (tid >> 2)) * COOP_PARAMS;
  const bool ok = coop_params_ok(pr);
  const uint32_t ia = ok ? pr[0] : 0, ib = ok ? pr[1] : 0, it = ok ? pr[2] : 0, times = ok ? pr[4] : 0;
  kg::coop_add_level<F>(img, COOP_ITEMS, nullptr, nullptr, ok && pr[3] != 0, ia, ib, it);
  kg::coop_dbl_level<F>(img, COOP_ITEMS, nullptr, nullptr, it, times, COOP_MAX_DBL);
  if (tid < COOP_ITEMS) {
    const size_t slot = g * COOP_ITEMS + tid;
    inf[slot] = (uint8_t)affine_out<F>(kg::coop_point(io, tid), o + slot * 2 * W);
  }
}
template <class F>
int run_coop(const uint32_t* items, const uint32_t* params, uint32_t* o, uint8_t* inf, size_t nwg) {
  constexpr int W = Conv<F>::W;
  const size_t n = nwg * COOP_ITEMS;
  Bufs B;
  const uint32_t *di = B.in(items, 4 * W * n), *dp = B.in(params, nwg * COOP_QUADS * COOP_PARAMS);
  uint32_t* dout = B.out<uint32_t>(2 * W * n);
  uint8_t* dinf = B.out<uint8_t>(n);
  if (B.ok()) { k_coop<F><<<(unsigned)nwg, NT>>>(di, dp, dout, dinf, nwg); B.launched(); }
  B.back(o, dout, 2 * W * n);
  B.back(inf, dinf, n);
  return (int)B.st;
}

// ---- the lane-pair Fq2 (fp2s.h): element i lives on lanes 2i (c0) and 2i + 1 (c1); NT is even, so a pair never straddles a workgroup ----------
using S2 = kg::Fp2S<Fq>;
enum Fp2sOp { S_MUL = 0, S_SQR, S_MUL2SUB, S_IS_ZERO, S_IS_ZERO_2P, S_ONE };
// a, b, c, d: 18 raw limbs per element (c0 | c1), taken as they are; out: 18 words per element, each lane writes its own nine (a verdict: the
// first of them, so that the two lanes' verdicts can be compared)
__global__ void __launch_bounds__(NT) k_fp2s_raw(int op, const uint32_t* a, const uint32_t* b, const uint32_t* c, const uint32_t* d, uint32_t* out, size_t n) {
  const size_t i = ((size_t)blockIdx.x * NT + threadIdx.x) >> 1;
  if (i >= n) return;                                    // whole pairs: both lanes of a pair leave together
  const size_t o = 18 * i + 9 * (size_t)S2::half();
  const S2 x{Raw<Fq>::limbs(a + o, nullptr)}, y{Raw<Fq>::limbs(b + o, nullptr)}, z{Raw<Fq>::limbs(c + o, nullptr)}, w{Raw<Fq>::limbs(d + o, nullptr)};
  S2 r = S2::zero();
  bool flag = false, limbs_out = true;
  switch (op) {
    case S_MUL: r = mul(x, y); break;
    case S_SQR: r = sqr(x); break;
    case S_MUL2SUB: r = mul2sub(x, y, z, w); break;
    case S_IS_ZERO: flag = is_zero(x); limbs_out = false; break;
    case S_IS_ZERO_2P: flag = is_zero_2p(x); limbs_out = false; break;
    case S_ONE: r = S2::one(); break;
    default: break;
  }
  if (limbs_out) { for (int k = 0; k < 9; ++k) out[o + k] = r.v.l[k]; }
  else out[o] = flag ? 1u : 0u;
}

// The stream formulas of curve.h on XYZZ<Fp2S<Fq>> through the reduction's own accessors (msm_reduce_kernels.h).  A point is 72 raw limbs:
// array of structures = the one-lane PointAoS<Fp2<Fq>> words (x.c0 x.c1 y.c0 ... zzz.c1), structure of arrays = word k of point i at [k * n + i].
// route 0: AosSrc, AosSrc -> AosDst (k_sum_tasks); 1: AosSrc, AosSrc -> SoaDst (k_gather_halve, k_gather_sum); 2: SoaSrc, SoaSrc -> SoaDst (k_halve).
// op 0 add_xyzz_stream, 1 double_xyzz_stream (of p), 2 copy_xyzz_stream (of p).  inplace: p is copied into the output slot first and the formula
// then runs with that slot as its first operand AND its destination, as the running sums of k_gather_sum / k_sum_tasks do.
// flags[i]: bit 0 the pair is active (an idle pair returns at once and writes nothing), bit 1 / bit 2 p / q is an EMPTY array-of-structures slot
// (AosSrc valid = false: the identity without a read).
enum { FL_ACTIVE = 1, FL_P_EMPTY = 2, FL_Q_EMPTY = 4 };
template <class A, class B, class Cur, class D>
__device__ __forceinline__ void fp2s_curve_case(int op, int inplace, const A& p, const B& q, const Cur& cur, D& dst) {
  if (op == 2) { kg::copy_xyzz_stream<S2>(p, dst); return; }
  if (!inplace) {
    if (op == 0) kg::add_xyzz_stream<S2>(p, q, dst); else kg::double_xyzz_stream<S2>(p, dst);
    return;
  }
  kg::copy_xyzz_stream<S2>(p, dst);
  KG_STREAM_FENCE();
  if (op == 0) kg::add_xyzz_stream<S2>(cur, q, dst); else kg::double_xyzz_stream<S2>(cur, dst);
}
template <int ROUTE>
__global__ void __launch_bounds__(NT) k_fp2s_curve(int op, int inplace, const uint32_t* p, const uint32_t* q, const uint8_t* flags, uint32_t* out, uint32_t n) {
  using namespace kg::msm;
  const uint32_t i = (blockIdx.x * (uint32_t)NT + threadIdx.x) >> 1;
  if (i >= n) return;
  const uint32_t f = flags[i];
  if (!(f & FL_ACTIVE)) return;
  constexpr uint32_t NWB = (uint32_t)kg::PointIO<S2>::NW * 4u;     // bytes per array-of-structures point
  const BufRsrc rp = soa_rsrc(p), rq = soa_rsrc(q), ro = soa_rsrc(out);
  const uint32_t s4 = n * 4u;
  if constexpr (ROUTE == 2) {
    const SoaSrc<S2> sp{rp, s4, i * 4u}, sq{rq, s4, i * 4u}, cur{ro, s4, i * 4u};
    SoaDst<S2> dst{ro, s4, i * 4u};
    fp2s_curve_case(op, inplace, sp, sq, cur, dst);
  } else {
    const AosSrc<S2> sp{rp, i * NWB, !(f & FL_P_EMPTY)}, sq{rq, i * NWB, !(f & FL_Q_EMPTY)};
    if constexpr (ROUTE == 0) {
      const AosSrc<S2> cur{ro, i * NWB, true};
      AosDst<S2> dst{ro, i * NWB};
      fp2s_curve_case(op, inplace, sp, sq, cur, dst);
    } else {
      const SoaSrc<S2> cur{ro, s4, i * 4u};
      SoaDst<S2> dst{ro, s4, i * 4u};
      fp2s_curve_case(op, inplace, sp, sq, cur, dst);
    }
  }
}

template <class F>
int run_raw(int op, const uint32_t* a, const uint32_t* b, const uint32_t* c, const uint32_t* d, const uint32_t* k, uint32_t* out, size_t n) {
  Bufs B;
  const uint32_t *da = B.in(a, 9 * n), *db = B.in(b, 9 * n), *dc = B.in(c, 9 * n), *dd = B.in(d, 9 * n), *dk = B.in(k, 18 * n);
  uint32_t* dout = B.out<uint32_t>(RAW_OUT * n);
  if (B.ok()) { k_raw<F><<<blocks(n), NT>>>(op, da, db, dc, dd, dk, dout, n); B.launched(); }
  B.back(out, dout, RAW_OUT * n);
  return (int)B.st;
}
template <class F>
int run_field(int op, const uint32_t* a, const uint32_t* b, uint32_t* o, size_t n) {
  constexpr int W = Conv<F>::W;
  Bufs B;
  const uint32_t *da = B.in(a, W * n), *db = B.in(b, W * n);
  uint32_t* dout = B.out<uint32_t>(W * n);
  if (B.ok()) { k_field<F><<<blocks(n), NT>>>(op, da, db, dout, n); B.launched(); }
  B.back(o, dout, W * n);
  return (int)B.st;
}
template <class F>
int run_curve(int op, const uint32_t* p, const uint32_t* q, uint32_t* o, uint8_t* inf, size_t n) {
  constexpr int W = Conv<F>::W;
  Bufs B;
  const uint32_t *dp = B.in(p, 4 * W * n), *dq = B.in(q, 4 * W * n);
  uint32_t* dout = B.out<uint32_t>(2 * W * n);
  uint8_t* dinf = B.out<uint8_t>(n);
  if (B.ok()) { k_curve<F><<<blocks(n), NT>>>(op, dp, dq, dout, dinf, n); B.launched(); }
  B.back(o, dout, 2 * W * n);
  B.back(inf, dinf, n);
  return (int)B.st;
}
template <class F, class SP>
int run_endo(const uint32_t* pts, uint32_t* o, size_t n) {
  constexpr int W = Conv<F>::W;
  Bufs B;
  const uint32_t* dp = B.in(pts, 2 * W * n);
  uint32_t* dout = B.out<uint32_t>(2 * W * n);
  if (B.ok()) { k_endo<F, SP><<<blocks(n), NT>>>(dp, dout, n); B.launched(); }
  B.back(o, dout, 2 * W * n);
  return (int)B.st;
}

}  // namespace

extern "C" {

// field: 0 Fr, 1 Fq; the arguments of ht_raw_ops (tests/host/hosttest.cpp) without the bounds
int dp_raw_ops(int field, int op, const uint32_t* a, const uint32_t* b, const uint32_t* c, const uint32_t* d, const uint32_t* k, uint32_t* out, size_t n) {
  if (n == 0) return 0;
  return field == 0 ? run_raw<Fr>(op, a, b, c, d, k, out, n) : run_raw<Fq>(op, a, b, c, d, k, out, n);
}
int dp_raw2_ops(int op, const uint32_t* a, const uint32_t* b, const uint32_t* c, const uint32_t* d, uint32_t* out, size_t n) {
  if (n == 0) return 0;
  Bufs B;
  const uint32_t *da = B.in(a, 18 * n), *db = B.in(b, 18 * n), *dc = B.in(c, 18 * n), *dd = B.in(d, 18 * n);
  uint32_t* dout = B.out<uint32_t>(RAW_OUT * n);
  if (B.ok()) { k_raw2<Fq><<<blocks(n), NT>>>(op, da, db, dc, dd, dout, n); B.launched(); }
  B.back(out, dout, RAW_OUT * n);
  return (int)B.st;
}
// Fp2S<Fq> on raw limbs (k_fp2s_raw): the operand arrays of dp_raw2_ops
int dp_fp2s_raw_ops(int op, const uint32_t* a, const uint32_t* b, const uint32_t* c, const uint32_t* d, uint32_t* out, size_t n) {
  if (n == 0) return 0;
  if (op < S_MUL || op > S_ONE) return -1;
  Bufs B;
  const uint32_t *da = B.in(a, 18 * n), *db = B.in(b, 18 * n), *dc = B.in(c, 18 * n), *dd = B.in(d, 18 * n);
  uint32_t* dout = B.out<uint32_t>(RAW_OUT * n);
  if (B.ok()) { k_fp2s_raw<<<blocks(2 * n), NT>>>(op, da, db, dc, dd, dout, n); B.launched(); }
  B.back(out, dout, RAW_OUT * n);
  return (int)B.st;
}
// the stream formulas on XYZZ<Fp2S<Fq>> (k_fp2s_curve); p, q, out: 72 n words each in the layout of the route; out goes in as the caller filled it
// (an idle pair leaves its slot as it was) and comes back
int dp_fp2s_curve_ops(int op, int route, int inplace, const uint32_t* p, const uint32_t* q, const uint8_t* flags, uint32_t* out, size_t n) {
  if (n == 0) return 0;
  if (op < 0 || op > 2 || route < 0 || route > 2 || n > ((size_t)1 << 20)) return -1;      // (72 words x 2^20 points: byte offsets stay below 2^32)
  Bufs B;
  const uint32_t *dp = B.in(p, 72 * n), *dq = B.in(q, 72 * n);
  const uint8_t* df = B.in(flags, n);
  uint32_t* dout = B.alloc<uint32_t>(72 * n);
  if (B.ok()) B.st = hipMemcpy(dout, out, 72 * n * sizeof(uint32_t), hipMemcpyHostToDevice);
  if (B.ok()) {
    if (route == 0) k_fp2s_curve<0><<<blocks(2 * n), NT>>>(op, inplace, dp, dq, df, dout, (uint32_t)n);
    else if (route == 1) k_fp2s_curve<1><<<blocks(2 * n), NT>>>(op, inplace, dp, dq, df, dout, (uint32_t)n);
    else k_fp2s_curve<2><<<blocks(2 * n), NT>>>(op, inplace, dp, dq, df, dout, (uint32_t)n);
    B.launched();
  }
  B.back(out, dout, 72 * n);
  return (int)B.st;
}
// field: 0 Fr, 1 Fq, 2 Fq2; the arguments of ht_field_ops (ABI-form elements)
int dp_field_ops(int field, int op, const uint32_t* a, const uint32_t* b, uint32_t* o, size_t n) {
  if (n == 0) return 0;
  if (field == 0) return run_field<Fr>(op, a, b, o, n);
  if (field == 1) return run_field<Fq>(op, a, b, o, n);
  return run_field<Fq2>(op, a, b, o, n);
}
// curve: 0 G1 (Fq), 1 Grumpkin (Fr), 2 G2 (Fq2); the arguments of ht_curve_ops
int dp_curve_ops(int curve, int op, const uint32_t* p, const uint32_t* q, uint32_t* o, uint8_t* inf, size_t n) {
  if (n == 0) return 0;
  if (curve == 0) return run_curve<Fq>(op, p, q, o, inf, n);
  if (curve == 1) return run_curve<Fr>(op, p, q, o, inf, n);
  return run_curve<Fq2>(op, p, q, o, inf, n);
}
// the arguments of ht_coop_ops: nwg waves of COOP_ITEMS items and 16 parameter rows each; o, inf: every item of every image, affine
int dp_coop_ops(int curve, const uint32_t* items, const uint32_t* params, size_t nwg, uint32_t* o, uint8_t* inf) {
  if (nwg == 0) return 0;
  if (curve == 0) return run_coop<Fq>(items, params, o, inf, nwg);
  if (curve == 1) return run_coop<Fr>(items, params, o, inf, nwg);
  return run_coop<Fq2>(items, params, o, inf, nwg);
}
// digits[i * 128 + w], w < ceil(255 / c)
int dp_small_digits(const uint32_t* k, size_t n, int c, int32_t* digits) {
  if (n == 0) return 0;
  Bufs B;
  const uint32_t* dk = B.in(k, 8 * n);
  int32_t* dd = B.out<int32_t>(128 * n);
  if (B.ok()) { k_small_digits<<<blocks(n), NT>>>(dk, n, c, dd); B.launched(); }
  B.back(digits, dd, 128 * n);
  return (int)B.st;
}
// field: the SCALAR field, 0 Fr (bn254 G1 / G2), 1 Fq (Grumpkin)
int dp_glv_decompose(int field, const uint32_t* k, size_t n, uint32_t* k1, uint32_t* k2, uint8_t* neg) {
  if (n == 0) return 0;
  Bufs B;
  const uint32_t* dk = B.in(k, 8 * n);
  uint32_t *d1 = B.out<uint32_t>(4 * n), *d2 = B.out<uint32_t>(4 * n);
  uint8_t* dn = B.out<uint8_t>(2 * n);
  if (B.ok()) {
    if (field == 0) k_glv_decompose<kg::GlvLattice<kg::FrParams>><<<blocks(n), NT>>>(dk, n, d1, d2, dn);
    else k_glv_decompose<kg::GlvLattice<kg::FqParams>><<<blocks(n), NT>>>(dk, n, d1, d2, dn);
    B.launched();
  }
  B.back(k1, d1, 4 * n);
  B.back(k2, d2, 4 * n);
  B.back(neg, dn, 2 * n);
  return (int)B.st;
}
// digits: [n][2][64]
int dp_glv_digits(int field, const uint32_t* k, size_t n, int c, int32_t* digits) {
  if (n == 0) return 0;
  Bufs B;
  const uint32_t* dk = B.in(k, 8 * n);
  int32_t* dd = B.out<int32_t>(128 * n);
  if (B.ok()) {
    if (field == 0) k_glv_digits<kg::GlvLattice<kg::FrParams>><<<blocks(n), NT>>>(dk, n, c, dd);
    else k_glv_digits<kg::GlvLattice<kg::FqParams>><<<blocks(n), NT>>>(dk, n, c, dd);
    B.launched();
  }
  B.back(digits, dd, 128 * n);
  return (int)B.st;
}
// msm::SmEndo<F, SP>::apply on affine points (x | y in the ABI form); curve: 0 G1, 1 Grumpkin, 2 G2
int dp_endo(int curve, const uint32_t* pts, uint32_t* o, size_t n) {
  if (n == 0) return 0;
  if (curve == 0) return run_endo<Fq, kg::FrParams>(pts, o, n);
  if (curve == 1) return run_endo<Fr, kg::FqParams>(pts, o, n);
  return run_endo<Fq2, kg::FrParams>(pts, o, n);
}

}  // extern "C"

// the integer kernels of the long MSM's scalar side, one at a time (dp_sort_*, dp_task_*, dp_level_ops)
#include "devprobe_sort.h"
// the point-side kernels of the long MSM, one at a time (dp_bases_*, dp_acc_tasks, dp_gather, dp_sum_tasks, dp_halve, dp_reduce_tail, dp_hot)
#include "devprobe_reduce.h"
