// LayerNorm kernels for the torch engine (SURVEY §2.2 model registry: every ConvNeXt, ViT, Swin and MaxViT block):
// a dense [rows][C] tensor normalised over C, C % 8 == 0, 8 <= C <= 2048, 64-bit row offsets.  x is 16-bit or fp32
// (ConvNeXt's residual stream), y / dy are 16-bit, dx has the dtype of x; gamma, beta, mean, rstd and the gamma / beta
// gradients are fp32.  One pass each way: the forward reads x and writes y (4 bytes per element for a 16-bit x), the
// backward reads dy and x and writes dx (6 bytes), with the gamma / beta gradients formed in the same walk.
//
// Work split: a row lives in registers.  L lanes (a power of two, a runtime argument) share a row and each holds NV
// <= 4 vectors of 8 channels (a template parameter); vector q * L + lane belongs to `lane`, so the L lanes of a row
// load consecutive 16 bytes (32 for an fp32 x) and vectors past C / 8 are masked.  A wave holds 64 / L rows, a
// 256-thread block a group of 256 / L; blocks are persistent and walk the groups with stride gridDim.x, loading the
// next group's raw vectors before they compute the current one (the row reductions would otherwise wait on memory
// with nothing else in flight).  gamma and beta for the lane's channels are loaded once per block.
//   * forward: mean = sum(x) / C by a per-lane chain and an xor-shuffle tree over the L lanes, then
//     var = sum((x - mean)^2) / C from the registers (two passes over registers, never E[x^2] - mean^2),
//     rstd = 1 / sqrt(var + eps), y = (x - mean) * rstd * gamma + beta rounded once.  No LDS.
//   * backward: xhat recomputed from the saved mean / rstd, the two row means through the same tree.  Every lane
//     keeps fp32 sums of dy * xhat and dy for its own channels over all rows it walks; at the end the row lanes of
//     a wave are folded by an xor-shuffle tree (strides 32 .. L), the four waves through LDS in a fixed order, and
//     the block writes one partial row [2][C] for wgrad_reduce: no atomics, bit-identical from run to run.  A
//     template flag drops the sums when gamma / beta need no gradient.
#include <cstdlib>

#include "../common.h"
#include "layernorm.h"

namespace pdt {

namespace {

// the raw 8 channels of one vector: 16 bytes of a 16-bit tensor, 32 of an fp32 one
template <bool F32>
struct LnRaw {
  uint4 v[F32 ? 2 : 1];
};

// `off` in elements; !ok reads nothing and yields zeros
template <bool F32>
PDT_DEVICE LnRaw<F32> ln_load(const void* p, int64_t off, bool ok) {
  LnRaw<F32> r;
#pragma unroll
  for (int i = 0; i < (F32 ? 2 : 1); ++i) r.v[i] = make_uint4(0u, 0u, 0u, 0u);
  if (ok) {
    if constexpr (F32) {
      const uint4* q = (const uint4*)((const float*)p + off);
      r.v[0] = q[0];
      r.v[1] = q[1];
    } else {
      r.v[0] = *(const uint4*)((const uint16_t*)p + off);
    }
  }
  return r;
}

template <int DT, bool F32>
PDT_DEVICE void ln_widen(const LnRaw<F32>& r, float (&o)[8]) {
  if constexpr (F32) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      o[4 * i] = __uint_as_float(r.v[i].x);
      o[4 * i + 1] = __uint_as_float(r.v[i].y);
      o[4 * i + 2] = __uint_as_float(r.v[i].z);
      o[4 * i + 3] = __uint_as_float(r.v[i].w);
    }
  } else {
    uint16_t h[8];
    unpack8(r.v[0], h);
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = E16<DT>::to_f(h[e]);
  }
}

template <int DT, bool F32>
PDT_DEVICE void ln_store(void* p, int64_t off, const float (&a)[8]) {
  if constexpr (F32) {
    uint4* q = (uint4*)((float*)p + off);
    q[0] = make_uint4(__float_as_uint(a[0]), __float_as_uint(a[1]), __float_as_uint(a[2]), __float_as_uint(a[3]));
    q[1] = make_uint4(__float_as_uint(a[4]), __float_as_uint(a[5]), __float_as_uint(a[6]), __float_as_uint(a[7]));
  } else {
    using E = E16<DT>;
    *(uint4*)((uint16_t*)p + off) =
        make_uint4(E::pack2(a[0], a[1]), E::pack2(a[2], a[3]), E::pack2(a[4], a[5]), E::pack2(a[6], a[7]));
  }
}

// sum over the L lanes of a row (lane ^ o stays inside the row's aligned group of L lanes); every lane gets the same
// bits: each level adds the same two values in both partners
PDT_DEVICE float ln_row_sum(float v, int L) {
  for (int o = L >> 1; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// geometry of a thread: lane l of row slot r; group g holds rows g * RB + r
struct LnThread {
  int l, r, RB;
};
PDT_DEVICE LnThread ln_thread(int L, int lshift) {
  return LnThread{(int)threadIdx.x & (L - 1), (int)threadIdx.x >> lshift, 256 >> lshift};
}

template <int DT, bool XF32, int NV>
__global__ __launch_bounds__(256) void layernorm_fwd_kernel(const void* __restrict__ x,
                                                            const float* __restrict__ gamma,
                                                            const float* __restrict__ beta, uint16_t* __restrict__ y,
                                                            float* __restrict__ mean, float* __restrict__ rstd,
                                                            int64_t rows, int64_t ngroups, int C, int L, int lshift,
                                                            float eps) {
  const LnThread t = ln_thread(L, lshift);
  const int nvec = C >> 3;
  bool vq[NV];
  float g[NV][8], b[NV][8];
#pragma unroll
  for (int q = 0; q < NV; ++q) {
    const int v = q * L + t.l;
    vq[q] = v < nvec;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      g[q][e] = vq[q] ? gamma[v * 8 + e] : 0.f;
      b[q][e] = vq[q] && beta != nullptr ? beta[v * 8 + e] : 0.f;
    }
  }
  const float fC = (float)C;

  LnRaw<XF32> cur[NV];
  {
    const int64_t row = (int64_t)blockIdx.x * t.RB + t.r;
#pragma unroll
    for (int q = 0; q < NV; ++q) cur[q] = ln_load<XF32>(x, row * C + (q * L + t.l) * 8, vq[q] && row < rows);
  }
  for (int64_t grp = blockIdx.x; grp < ngroups; grp += gridDim.x) {  // uniform per block: every lane shuffles
    const int64_t row = grp * t.RB + t.r;
    const int64_t nrow = row + (int64_t)gridDim.x * t.RB;
    LnRaw<XF32> nxt[NV];
#pragma unroll
    for (int q = 0; q < NV; ++q) nxt[q] = ln_load<XF32>(x, nrow * C + (q * L + t.l) * 8, vq[q] && nrow < rows);

    float xf[NV][8];
    float s = 0.f;
#pragma unroll
    for (int q = 0; q < NV; ++q) {
      ln_widen<DT, XF32>(cur[q], xf[q]);  // zeros where masked
#pragma unroll
      for (int e = 0; e < 8; ++e) s += xf[q][e];
    }
    const float mu = ln_row_sum(s, L) / fC;
    float ss = 0.f;
#pragma unroll
    for (int q = 0; q < NV; ++q) {
      if (vq[q]) {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          xf[q][e] -= mu;
          ss += xf[q][e] * xf[q][e];
        }
      }
    }
    const float rs = 1.f / sqrtf(ln_row_sum(ss, L) / fC + eps);
    if (row < rows) {
#pragma unroll
      for (int q = 0; q < NV; ++q) {
        if (vq[q]) {
          float o[8];
#pragma unroll
          for (int e = 0; e < 8; ++e) o[e] = xf[q][e] * rs * g[q][e] + b[q][e];
          ln_store<DT, false>(y, row * C + (q * L + t.l) * 8, o);
        }
      }
      if (t.l == 0) {
        mean[row] = mu;
        rstd[row] = rs;
      }
    }
#pragma unroll
    for (int q = 0; q < NV; ++q) cur[q] = nxt[q];
  }
}

template <int DT, bool XF32, int NV, bool AFFINE>
__global__ __launch_bounds__(256) void layernorm_bwd_kernel(const uint16_t* __restrict__ dy,
                                                            const void* __restrict__ x,
                                                            const float* __restrict__ mean,
                                                            const float* __restrict__ rstd,
                                                            const float* __restrict__ gamma, void* __restrict__ dx,
                                                            float* __restrict__ partials, int64_t rows,
                                                            int64_t ngroups, int C, int L, int lshift) {
  const LnThread t = ln_thread(L, lshift);
  const int nvec = C >> 3;
  bool vq[NV];
  float g[NV][8], dg[NV][8], db[NV][8];
#pragma unroll
  for (int q = 0; q < NV; ++q) {
    const int v = q * L + t.l;
    vq[q] = v < nvec;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      g[q][e] = vq[q] ? gamma[v * 8 + e] : 0.f;
      dg[q][e] = 0.f;
      db[q][e] = 0.f;
    }
  }
  const float fC = (float)C;

  LnRaw<XF32> cx[NV];
  LnRaw<false> cd[NV];
  float cmu, crs;
  {
    const int64_t row = (int64_t)blockIdx.x * t.RB + t.r;
    const bool ok = row < rows;
#pragma unroll
    for (int q = 0; q < NV; ++q) {
      cx[q] = ln_load<XF32>(x, row * C + (q * L + t.l) * 8, vq[q] && ok);
      cd[q] = ln_load<false>(dy, row * C + (q * L + t.l) * 8, vq[q] && ok);
    }
    cmu = ok ? mean[row] : 0.f;
    crs = ok ? rstd[row] : 0.f;
  }
  for (int64_t grp = blockIdx.x; grp < ngroups; grp += gridDim.x) {
    const int64_t row = grp * t.RB + t.r;
    const int64_t nrow = row + (int64_t)gridDim.x * t.RB;
    const bool nok = nrow < rows;
    LnRaw<XF32> nx[NV];
    LnRaw<false> nd[NV];
#pragma unroll
    for (int q = 0; q < NV; ++q) {
      nx[q] = ln_load<XF32>(x, nrow * C + (q * L + t.l) * 8, vq[q] && nok);
      nd[q] = ln_load<false>(dy, nrow * C + (q * L + t.l) * 8, vq[q] && nok);
    }
    const float nmu = nok ? mean[nrow] : 0.f, nrs = nok ? rstd[nrow] : 0.f;

    // a row past the end holds zeros with mean = rstd = 0: xhat = a = 0, nothing is added anywhere
    float xh[NV][8], a[NV][8];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int q = 0; q < NV; ++q) {
      float d[8];
      ln_widen<DT, XF32>(cx[q], xh[q]);
      ln_widen<DT, false>(cd[q], d);
      if (vq[q]) {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          xh[q][e] = (xh[q][e] - cmu) * crs;
          a[q][e] = g[q][e] * d[e];
          s1 += a[q][e];
          s2 += a[q][e] * xh[q][e];
          if constexpr (AFFINE) {
            dg[q][e] += d[e] * xh[q][e];
            db[q][e] += d[e];
          }
        }
      }
    }
    const float m1 = ln_row_sum(s1, L) / fC, m2 = ln_row_sum(s2, L) / fC;
    if (row < rows) {
#pragma unroll
      for (int q = 0; q < NV; ++q) {
        if (vq[q]) {
          float o[8];
#pragma unroll
          for (int e = 0; e < 8; ++e) o[e] = crs * (a[q][e] - m1 - xh[q][e] * m2);
          ln_store<DT, XF32>(dx, row * C + (q * L + t.l) * 8, o);
        }
      }
    }
#pragma unroll
    for (int q = 0; q < NV; ++q) {
      cx[q] = nx[q];
      cd[q] = nd[q];
    }
    cmu = nmu;
    crs = nrs;
  }

  if constexpr (AFFINE) {
    // red[wave][channel]: channel (q * L + l) * 8 + e < NV * 512; every channel < C is written by all four waves
    __shared__ float red[4][NV * 512];
    const int wave = threadIdx.x >> 6, wl = threadIdx.x & 63;
    float* out = partials + (int64_t)blockIdx.x * 2 * C;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
#pragma unroll
      for (int q = 0; q < NV; ++q) {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          float v = k == 0 ? dg[q][e] : db[q][e];
          for (int o = 32; o >= L; o >>= 1) v += __shfl_xor(v, o, 64);  // the wave's 64 / L row slots
          if (wl < L) red[wave][(q * L + t.l) * 8 + e] = v;
        }
      }
      __syncthreads();
      for (int c = threadIdx.x; c < C; c += 256) out[k * C + c] = (red[0][c] + red[1][c]) + (red[2][c] + red[3][c]);
      __syncthreads();
    }
  }
}

void check_args(const char* what, int dtype, int64_t rows, int C, const LnPlan& p) {
  const bool pow2 = p.L >= 1 && p.L <= 64 && (p.L & (p.L - 1)) == 0;
  if ((dtype != kBF16 && dtype != kF16) || C < 8 || C > 2048 || C % 8 != 0 || rows < 1 ||
      rows * C >= (int64_t(1) << 40) || !pow2 || p.NV < 1 || p.NV > 4 || p.L * p.NV < C / 8 || p.blocks < 1)
    pdt_hip_fail(what, hipErrorInvalidValue, __FILE__, __LINE__);
}

int ilog2(int v) {
  int s = 0;
  while ((1 << s) < v) ++s;
  return s;
}

}  // namespace

LnPlan layernorm_plan(int64_t rows, int C, int max_blocks) {
  // The fewest vectors per lane, then the fewest idle lanes: C = 96 as L = 16, NV = 1.  PDT_LN_TIGHT=1 swaps the two
  // criteria (C = 96 as L = 4, NV = 3: no idle lanes), the A/B of profiles/layernorm_mi355x.md, which it lost: three
  // vectors per lane cost the backward its occupancy.
  static const bool wide = [] {
    const char* e = getenv("PDT_LN_TIGHT");
    return !(e && e[0] == '1');
  }();
  const int nvec = C / 8;
  LnPlan p{64, 4, 1};
  int best_idle = 1 << 30, best_nv = 1 << 30;
  for (int L = 64; L >= 1; L >>= 1) {
    const int nv = (nvec + L - 1) / L;
    if (nv > 4) break;
    const int idle = L * nv - nvec;
    const bool better = wide ? (nv < best_nv || (nv == best_nv && idle < best_idle))
                             : (idle < best_idle || (idle == best_idle && nv < best_nv));
    if (better) {
      p.L = L;
      p.NV = nv;
      best_idle = idle;
      best_nv = nv;
    }
  }
  // equal walks: the blocks that give every block the same number of groups (the last may have fewer); above 64 a
  // multiple of 32, so the partial rows fold in two short wgrad_reduce stages -- rounded up where max_blocks allows
  // (a block without a group writes a zero partial row), else down (some blocks walk one group more)
  const int64_t rb = 256 / p.L, groups = (rows + rb - 1) / rb;
  const int64_t cap = max_blocks < 1 ? 1 : max_blocks;
  const int64_t per = (groups + cap - 1) / cap;
  int64_t blocks = per > 0 ? (groups + per - 1) / per : 1;
  if (blocks > 64) blocks = (blocks + 31) / 32 * 32 <= cap ? (blocks + 31) / 32 * 32 : blocks / 32 * 32;
  p.blocks = (int)(blocks < 1 ? 1 : blocks);
  return p;
}

#define PDT_LN_NV(KERNEL, ...)                                                                                     \
  switch (plan.NV) {                                                                                               \
    case 1: KERNEL(1, __VA_ARGS__); break;                                                                         \
    case 2: KERNEL(2, __VA_ARGS__); break;                                                                         \
    case 3: KERNEL(3, __VA_ARGS__); break;                                                                         \
    default: KERNEL(4, __VA_ARGS__); break;                                                                        \
  }

void layernorm_fwd_launch(int dtype, bool x_f32, const void* x, const float* gamma, const float* beta, uint16_t* y,
                          float* mean, float* rstd, int64_t rows, int C, float eps, const LnPlan& plan,
                          hipStream_t s) {
  check_args("layernorm_fwd_launch: arguments outside the kernels' contract", dtype, rows, C, plan);
  PDT_COUNT("layernorm_fwd");
  const int64_t rb = 256 / plan.L, ngroups = (rows + rb - 1) / rb;
  const int lshift = ilog2(plan.L);
#define PDT_LN_F(NVv, DTv, XFv)                                                                                    \
  hipLaunchKernelGGL((layernorm_fwd_kernel<DTv, XFv, NVv>), dim3((unsigned)plan.blocks), dim3(256), 0, s, x, gamma, \
                     beta, y, mean, rstd, rows, ngroups, C, plan.L, lshift, eps)
  if (dtype == kBF16) {
    if (x_f32) { PDT_LN_NV(PDT_LN_F, kBF16, true) } else { PDT_LN_NV(PDT_LN_F, kBF16, false) }
  } else {
    if (x_f32) { PDT_LN_NV(PDT_LN_F, kF16, true) } else { PDT_LN_NV(PDT_LN_F, kF16, false) }
  }
#undef PDT_LN_F
}

void layernorm_bwd_launch(int dtype, bool x_f32, const uint16_t* dy, const void* x, const float* mean,
                          const float* rstd, const float* gamma, void* dx, float* partials, int64_t rows, int C,
                          const LnPlan& plan, hipStream_t s) {
  check_args("layernorm_bwd_launch: arguments outside the kernels' contract", dtype, rows, C, plan);
  PDT_COUNT("layernorm_bwd");
  const int64_t rb = 256 / plan.L, ngroups = (rows + rb - 1) / rb;
  const int lshift = ilog2(plan.L);
#define PDT_LN_B(NVv, DTv, XFv, AFv)                                                                               \
  hipLaunchKernelGGL((layernorm_bwd_kernel<DTv, XFv, NVv, AFv>), dim3((unsigned)plan.blocks), dim3(256), 0, s, dy, \
                     x, mean, rstd, gamma, dx, partials, rows, ngroups, C, plan.L, lshift)
#define PDT_LN_BX(DTv, AFv)                                                                                        \
  if (x_f32) { PDT_LN_NV(PDT_LN_B, DTv, true, AFv) } else { PDT_LN_NV(PDT_LN_B, DTv, false, AFv) }
  if (dtype == kBF16) {
    if (partials) { PDT_LN_BX(kBF16, true) } else { PDT_LN_BX(kBF16, false) }
  } else {
    if (partials) { PDT_LN_BX(kF16, true) } else { PDT_LN_BX(kF16, false) }
  }
#undef PDT_LN_BX
#undef PDT_LN_B
}
#undef PDT_LN_NV

}  // namespace pdt
