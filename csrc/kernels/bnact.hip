// Fused BatchNorm + activation over NHWC 16-bit activations viewed as [rows = N*H*W, C], fp32 math: the training
// passes of the torch engine's BNAct2d (pytorch_distributed_template_amd/ops/bnact.py, --native-bnact on).
//
// Forward:  bnact_stats (per-channel sum x, sum x^2 -> fp64 slots) -> bn_finalize_slots (bn.hip: coef =
//           [scale | shift | mean | invstd], running statistics) -> bnact_fwd (out = act(u), u = fma(x, scale, shift)).
// Backward: bnact_bwd_reduce (u recomputed from x, dz = g * act'(u); sum dz, sum dz * xhat -> fp64 slots)
//           -> bn_slot_sum -> bn_bwd_finalize (bn.hip: dgamma, dbeta, bcoef = [A | B | Cc])
//           -> bnact_bwd_apply (dz recomputed the same way, dx = A*dz + B*x + Cc).
// The BN output is never materialised: the backward reads x and g only.  Forward and backward evaluate the same
// fp32 u (one explicit fmaf), so they always agree on the activation's branch.
//
// Thread mapping (all four kernels): a thread owns ONE fixed group of 8 consecutive channels and walks rows, so its
// per-channel coefficients are loaded once, for every C % 8 == 0 (not only the powers of two bn.hip hoists).  A
// 256-thread block is cvb channel groups x rpi row lanes; a row of C / 8 groups is split into `chunks` column
// chunks of cvb groups (grid.y).  bnact_plan picks cvb so that few lanes idle for widths that do not divide 256:
// C = 1280 (160 groups) runs as 5 chunks of 32 groups x 8 row lanes, C = 24 as 3 groups x 85 row lanes.
// The lanes and the deterministic statistics (per-thread fp32 chains, fixed-order LDS sum over the block's row
// lanes, one partial row per row block, stat_rows_reduce into the fp64 slots) are col_reduce.h's, shared with
// the BN-backward and pooled reduces.
#include "../common.h"
#include "bnact.h"
#include "col_reduce.h"

namespace pdt {

BnActPlan bnact_plan(int64_t rows, int C) {
  const int vpr = C / 8;
  // candidates: at least 8 groups (128 contiguous bytes per row segment) unless the whole row is narrower
  const int lo = vpr < 8 ? vpr : 8, hi = vpr < 256 ? vpr : 256;
  int best = hi;
  int64_t best_num = -1, best_den = 1;
  for (int cvb = lo; cvb <= hi; ++cvb) {
    const int rpi = 256 / cvb, chunks = (vpr + cvb - 1) / cvb;
    // share of launched lanes that own data: vpr * rpi of chunks * 256 (ties: the wider chunk)
    const int64_t num = (int64_t)vpr * rpi, den = (int64_t)chunks * 256;
    if (best_num < 0 || num * best_den >= best_num * den) {
      best_num = num;
      best_den = den;
      best = cvb;
    }
  }
  // reduce kernels: >= 16 rows per thread, at most 2048 blocks in all
  const int chunks = (vpr + best - 1) / best;
  return col_plan(rows, C, 8, 2, 16, 2048 / chunks > 0 ? 2048 / chunks : 1, best);
}

namespace {

constexpr int kU = 4;   // rows per thread of the elementwise kernels, all loads issued before any math
constexpr int kRU = 4;  // rows per loop iteration of bnact_stats
constexpr int kBU = 2;  // ... of bnact_bwd_reduce (two operands per row)

PDT_DEVICE void load8(const float* __restrict__ p, float (&v)[8]) {
  const float4 a = *(const float4*)p, b = *(const float4*)(p + 4);
  v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
  v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
}

// torch's conventions: relu' = 1 iff u > 0; relu6' = 1 iff 0 < u < 6; hardswish' = 0 for u <= -3, (2u + 3) / 6 for
// -3 < u < 3, 1 from 3 on (aten's hardswish_backward).  NaN passes through the forward.
template <int ACT>
PDT_DEVICE float act_fwd(float u) {
  if constexpr (ACT == kActRelu) return u <= 0.f ? 0.f : u;
  if constexpr (ACT == kActRelu6) return u <= 0.f ? 0.f : (u >= 6.f ? 6.f : u);
  if constexpr (ACT == kActHardswish) return u * fminf(fmaxf(u + 3.f, 0.f), 6.f) / 6.f;
  return u;
}

template <int ACT>
PDT_DEVICE float act_bwd(float u, float g) {
  if constexpr (ACT == kActRelu) return u > 0.f ? g : 0.f;
  if constexpr (ACT == kActRelu6) return (u > 0.f && u < 6.f) ? g : 0.f;
  if constexpr (ACT == kActHardswish) {
    if (u <= -3.f) return 0.f;
    if (u < 3.f) return g * (fmaf(2.f, u, 3.f) / 6.f);
    return g;
  }
  return g;
}

// ------------------------------------------------------------------------------------------------- statistics
template <int DT, bool NT>
__global__ __launch_bounds__(256) void bnact_stats_kernel(const uint16_t* __restrict__ x, float* __restrict__ srows,
                                                          int64_t rows, int C, int cvb, int rpi) {
  using E = E16<DT>;
  __shared__ float red[256 * 8 * 2];
  const ColLane ln = col_lanes<8>(C, cvb, rpi);
  float s[2][8];
#pragma unroll
  for (int e = 0; e < 8; ++e) s[0][e] = s[1][e] = 0.f;
  if (ln.active) {
    const int64_t stride = (int64_t)gridDim.x * rpi;
    for (int64_t r = (int64_t)blockIdx.x * rpi + ln.rl; r < rows; r += stride * kRU) {
      uint4 v[kRU];
#pragma unroll
      for (int j = 0; j < kRU; ++j)
        if (r + j * stride < rows) v[j] = ld16<NT>(x + (r + j * stride) * C + ln.c0);
#pragma unroll
      for (int j = 0; j < kRU; ++j) {
        if (r + j * stride >= rows) break;
        uint16_t h[8];
        unpack8(v[j], h);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float f = E::to_f(h[e]);
          s[0][e] += f;
          s[1][e] = fmaf(f, f, s[1][e]);  // the square of a 16-bit value is exact in fp32
        }
      }
    }
  }
  block_rows_out<2>(s, ln, red, srows, C, cvb, rpi);
}

// ---------------------------------------------------------------------------------------------------- forward
template <int DT, int ACT, bool NT>
__global__ __launch_bounds__(256) void bnact_fwd_kernel(const uint16_t* __restrict__ x, const float* __restrict__ coef,
                                                        uint16_t* __restrict__ out, int64_t rows, int C, int cvb,
                                                        int rpi) {
  using E = E16<DT>;
  const ColLane ln = col_lanes<8>(C, cvb, rpi);
  if (!ln.active) return;
  const int64_t r0 = (int64_t)blockIdx.x * (kU * rpi) + ln.rl;
  uint4 v[kU];
#pragma unroll
  for (int u = 0; u < kU; ++u)
    if (r0 + u * rpi < rows) v[u] = ld16<NT>(x + (r0 + u * rpi) * C + ln.c0);
  float sc[8], sh[8];
  load8(coef + ln.c0, sc);
  load8(coef + C + ln.c0, sh);
#pragma unroll
  for (int u = 0; u < kU; ++u) {
    const int64_t r = r0 + u * rpi;
    if (r >= rows) break;
    uint16_t h[8];
    unpack8(v[u], h);
    uint32_t o[4];
#pragma unroll
    for (int e = 0; e < 4; ++e)
      o[e] = E::pack2(act_fwd<ACT>(fmaf(E::to_f(h[2 * e]), sc[2 * e], sh[2 * e])),
                      act_fwd<ACT>(fmaf(E::to_f(h[2 * e + 1]), sc[2 * e + 1], sh[2 * e + 1])));
    st16<NT>(out + r * C + ln.c0, make_uint4(o[0], o[1], o[2], o[3]));
  }
}

// ------------------------------------------------------------------------------------------- backward reduce
template <int DT, int ACT, bool NT>
__global__ __launch_bounds__(256) void bnact_bwd_reduce_kernel(const uint16_t* __restrict__ g,
                                                               const uint16_t* __restrict__ x,
                                                               const float* __restrict__ coef,
                                                               float* __restrict__ srows, int64_t rows, int C, int cvb,
                                                               int rpi) {
  using E = E16<DT>;
  __shared__ float red[256 * 8 * 2];
  const ColLane ln = col_lanes<8>(C, cvb, rpi);
  float s[2][8];
#pragma unroll
  for (int e = 0; e < 8; ++e) s[0][e] = s[1][e] = 0.f;
  if (ln.active) {
    float sc[8], sh[8], mean[8], inv[8];
    if constexpr (ACT != kActIdentity) {
      load8(coef + ln.c0, sc);
      load8(coef + C + ln.c0, sh);
    }
    load8(coef + 2 * C + ln.c0, mean);
    load8(coef + 3 * C + ln.c0, inv);
    const int64_t stride = (int64_t)gridDim.x * rpi;
    for (int64_t r = (int64_t)blockIdx.x * rpi + ln.rl; r < rows; r += stride * kBU) {
      uint4 gv[kBU], xv[kBU];
#pragma unroll
      for (int j = 0; j < kBU; ++j)
        if (r + j * stride < rows) {
          gv[j] = ld16<NT>(g + (r + j * stride) * C + ln.c0);
          xv[j] = ld16<NT>(x + (r + j * stride) * C + ln.c0);
        }
#pragma unroll
      for (int j = 0; j < kBU; ++j) {
        if (r + j * stride >= rows) break;
        uint16_t gh[8], xh[8];
        unpack8(gv[j], gh);
        unpack8(xv[j], xh);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float xf = E::to_f(xh[e]);
          float dz = E::to_f(gh[e]);
          if constexpr (ACT != kActIdentity) dz = act_bwd<ACT>(fmaf(xf, sc[e], sh[e]), dz);
          s[0][e] += dz;
          s[1][e] += dz * ((xf - mean[e]) * inv[e]);
        }
      }
    }
  }
  block_rows_out<2>(s, ln, red, srows, C, cvb, rpi);
}

// -------------------------------------------------------------------------------------------- backward apply
template <int DT, int ACT, bool NT>
__global__ __launch_bounds__(256) void bnact_bwd_apply_kernel(const uint16_t* __restrict__ g,
                                                              const uint16_t* __restrict__ x,
                                                              const float* __restrict__ coef,
                                                              const float* __restrict__ bcoef,
                                                              uint16_t* __restrict__ dx, int64_t rows, int C, int cvb,
                                                              int rpi) {
  using E = E16<DT>;
  const ColLane ln = col_lanes<8>(C, cvb, rpi);
  if (!ln.active) return;
  const int64_t r0 = (int64_t)blockIdx.x * (kU * rpi) + ln.rl;
  uint4 gv[kU], xv[kU];
#pragma unroll
  for (int u = 0; u < kU; ++u)
    if (r0 + u * rpi < rows) {
      gv[u] = ld16<NT>(g + (r0 + u * rpi) * C + ln.c0);
      xv[u] = ld16<NT>(x + (r0 + u * rpi) * C + ln.c0);
    }
  float sc[8], sh[8], A[8], B[8], Cc[8];
  if constexpr (ACT != kActIdentity) {
    load8(coef + ln.c0, sc);
    load8(coef + C + ln.c0, sh);
  }
  load8(bcoef + ln.c0, A);
  load8(bcoef + C + ln.c0, B);
  load8(bcoef + 2 * C + ln.c0, Cc);
#pragma unroll
  for (int u = 0; u < kU; ++u) {
    const int64_t r = r0 + u * rpi;
    if (r >= rows) break;
    uint16_t gh[8], xh[8];
    unpack8(gv[u], gh);
    unpack8(xv[u], xh);
    float d[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float xf = E::to_f(xh[e]);
      float dz = E::to_f(gh[e]);
      if constexpr (ACT != kActIdentity) dz = act_bwd<ACT>(fmaf(xf, sc[e], sh[e]), dz);
      d[e] = fmaf(A[e], dz, fmaf(B[e], xf, Cc[e]));
    }
    st16<NT>(dx + r * C + ln.c0, make_uint4(E::pack2(d[0], d[1]), E::pack2(d[2], d[3]), E::pack2(d[4], d[5]),
                                            E::pack2(d[6], d[7])));
  }
}

dim3 ew_grid(int64_t rows, const BnActPlan& p) {
  const int64_t per = (int64_t)kU * p.rpi, b = (rows + per - 1) / per;
  if (b >= (int64_t(1) << 31)) pdt_hip_fail("bnact: tensor too large", hipErrorInvalidValue, __FILE__, __LINE__);
  return dim3((unsigned)(b < 1 ? 1 : b), p.chunks);
}

}  // namespace

// dispatch KERNEL<DT, ACT, NT> over the runtime (dtype, act, nt); falls through when nothing matches
#define PDT_BNACT_CASE(KERNEL, DT_, ACT_, NT_, grid, ...)                                                \
  if (dtype == DT_ && act == ACT_ && nt == NT_) {                                                        \
    hipLaunchKernelGGL((KERNEL<DT_, ACT_, NT_>), grid, dim3(256), 0, s, __VA_ARGS__);                    \
    launched_ = true;                                                                                    \
  }
#define PDT_BNACT_ACTS(KERNEL, DT_, NT_, grid, ...)                                                      \
  PDT_BNACT_CASE(KERNEL, DT_, kActIdentity, NT_, grid, __VA_ARGS__)                                      \
  PDT_BNACT_CASE(KERNEL, DT_, kActRelu, NT_, grid, __VA_ARGS__)                                          \
  PDT_BNACT_CASE(KERNEL, DT_, kActRelu6, NT_, grid, __VA_ARGS__)                                         \
  PDT_BNACT_CASE(KERNEL, DT_, kActHardswish, NT_, grid, __VA_ARGS__)
#define PDT_BNACT_DISPATCH(KERNEL, grid, ...)                                                            \
  bool launched_ = false;                                                                                \
  PDT_BNACT_ACTS(KERNEL, kBF16, false, grid, __VA_ARGS__)                                                \
  PDT_BNACT_ACTS(KERNEL, kBF16, true, grid, __VA_ARGS__)                                                 \
  PDT_BNACT_ACTS(KERNEL, kF16, false, grid, __VA_ARGS__)                                                 \
  PDT_BNACT_ACTS(KERNEL, kF16, true, grid, __VA_ARGS__)

void bnact_stats_launch(int dtype, const uint16_t* x, double* slots, int64_t rows, int C, const BnActPlan& p,
                        hipStream_t s) {
  PDT_COUNT("bnact_stats");
  const bool nt = ew_nt(rows * C * 2);
  const dim3 grid(p.blocks, p.chunks);
  col_reduce_run(p.blocks, C, 2, slots, s, [&](float* srows) {
#define PDT_ST(DT_, NT_)                                                                                 \
  if (dtype == DT_ && nt == NT_) {                                                                       \
    hipLaunchKernelGGL((bnact_stats_kernel<DT_, NT_>), grid, dim3(256), 0, s, x, srows, rows, C, p.cvb, p.rpi); \
    return;                                                                                              \
  }
    PDT_ST(kBF16, false) PDT_ST(kBF16, true) PDT_ST(kF16, false) PDT_ST(kF16, true)
#undef PDT_ST
    pdt_hip_fail("bnact_stats: unsupported variant", hipErrorInvalidValue, __FILE__, __LINE__);
  });
}

void bnact_fwd_launch(int dtype, int act, const uint16_t* x, const float* coef, uint16_t* out, int64_t rows, int C,
                      const BnActPlan& p, hipStream_t s) {
  PDT_COUNT("bnact_fwd");
  const bool nt = ew_nt(rows * C * 2);
  const dim3 grid = ew_grid(rows, p);
  PDT_BNACT_DISPATCH(bnact_fwd_kernel, grid, x, coef, out, rows, C, p.cvb, p.rpi)
  if (!launched_) pdt_hip_fail("bnact_fwd: unsupported variant", hipErrorInvalidValue, __FILE__, __LINE__);
}

void bnact_bwd_reduce_launch(int dtype, int act, const uint16_t* g, const uint16_t* x, const float* coef, double* slots,
                             int64_t rows, int C, const BnActPlan& p, hipStream_t s) {
  PDT_COUNT("bnact_bwd_reduce");
  const bool nt = ew_nt(rows * C * 2);
  const dim3 grid(p.blocks, p.chunks);
  col_reduce_run(p.blocks, C, 2, slots, s, [&](float* srows) {
    PDT_BNACT_DISPATCH(bnact_bwd_reduce_kernel, grid, g, x, coef, srows, rows, C, p.cvb, p.rpi)
    if (!launched_) pdt_hip_fail("bnact_bwd_reduce: unsupported variant", hipErrorInvalidValue, __FILE__, __LINE__);
  });
}

void bnact_bwd_apply_launch(int dtype, int act, const uint16_t* g, const uint16_t* x, const float* coef,
                            const float* bcoef, uint16_t* dx, int64_t rows, int C, const BnActPlan& p, hipStream_t s) {
  PDT_COUNT("bnact_bwd_apply");
  const bool nt = ew_nt(rows * C * 2);
  const dim3 grid = ew_grid(rows, p);
  PDT_BNACT_DISPATCH(bnact_bwd_apply_kernel, grid, g, x, coef, bcoef, dx, rows, C, p.cvb, p.rpi)
  if (!launched_) pdt_hip_fail("bnact_bwd_apply: unsupported variant", hipErrorInvalidValue, __FILE__, __LINE__);
}

}  // namespace pdt
