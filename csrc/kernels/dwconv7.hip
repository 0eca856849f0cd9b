// 7x7 depthwise convolution kernels (SURVEY §2.2 model registry: ConvNeXt's CNBlock conv): groups == Cin == Cout == C,
// kernel K x K = 7 x 7, stride 1, padding 3, dilation 1, C % 8 == 0, optional per-channel bias.  NHWC 16-bit
// activations, taps-major [K][K][C] 16-bit weight (one tap's 8 channels = one 16-byte load, the layout of dwconv.hip),
// fp32 accumulation, one rounding of the output, 64-bit image bases (everything inside one image is 32-bit).
//
// Plain VALU work: a depthwise conv has no reduction shared between channels, so there is no matrix product for an
// MFMA to compute -- every multiply-add belongs to exactly one (pixel, channel) output.  What the design buys is data
// movement: dwconv.hip's strip kernel keeps all K * K taps in registers (196 VGPRs packed at 7 x 7) and re-reads
// every input vector from global memory once per tap column; here the input halo is staged in LDS once and a register
// window walks it.
//   * dwconv7_tile: forward, and the backward data (the same conv over dy with the taps flipped and no bias).  A
//     256-thread block owns TH output rows x TW output columns x CVB channel vectors and stages the
//     (TH + 6) x (TW + 6) x CVB halo with 16-byte loads (padding and positions past the tensor are written as +0 and
//     never read from memory).  Thread = (channel vector, output column), channel vector fastest: the lanes of a
//     wave read consecutive 16 bytes of LDS, so ds_read_b128 is conflict-free (tools/lds_sim.py dwconv7).  The loop is
//     over the 7 tap columns s: only w[0..6][s] are live (56 fp32 VGPRs), the thread walks the TH + 6 halo rows of
//     column q + s, reads each LDS vector once and feeds every output row it touches: 7 * (TH + 6) LDS reads per TH
//     outputs.  Three shapes TW x CVB = 32 x 8, 16 x 16, 8 x 32, chosen from W alone.
//   * dwconv7_wgrad: weight gradient with the bias gradient.  A block owns 8 channel vectors and its split's pixel
//     range, walked in bands of up to BR output rows x WC columns whose x halo and dy rows are staged in LDS once.
//     Thread = (channel vector, row slot 0..7, pixel lane 0..3): slots 0..6 are the kernel rows r, slot 7 sums dy.  A
//     thread walks its lane's rows along q with a 7-wide register window of the x row p + r - 3: one new LDS read of
//     x and one of dy per step, then 56 FMAs.  Fixed summation order (pixels in order, lanes in lane order through
//     LDS), one fp32 slab [split][50][C] per block for wgrad_reduce: no atomics, bit-identical from run to run.
#include "../common.h"
#include "dwconv7.h"

namespace pdt {

namespace {

template <int DT>
PDT_DEVICE void unpack8f7(uint4 v, float (&o)[8]) {
  uint16_t h[8];
  unpack8(v, h);
#pragma unroll
  for (int e = 0; e < 8; ++e) o[e] = E16<DT>::to_f(h[e]);
}

template <int DT>
PDT_DEVICE uint4 pack8f7(const float (&a)[8]) {
  using E = E16<DT>;
  return make_uint4(E::pack2(a[0], a[1]), E::pack2(a[2], a[3]), E::pack2(a[4], a[5]), E::pack2(a[6], a[7]));
}

// Output rows per tile of dwconv7_tile for a tile TW columns wide: the halo must leave two blocks per CU in the
// 160 KiB of LDS ((TH + 6) * (TW + 6) * (256 / TW) * 16 bytes: 68096, 78848 and 71680), and 8 x 32 serves the
// 7-row maps (profiles/dwconv7_mi355x.md has the resource table and the strip-height A/B).
#ifndef PDT_DW7_TH
#define PDT_DW7_TH 8  // rows of the 32- and 16-column tiles (-DPDT_DW7_TH=4: the A/B build of the profile)
#endif
template <int TW> constexpr int tile_th() { return TW == 8 ? 4 : PDT_DW7_TH; }

// y[n][p][q][c] = bias[c] + sum_{r,s} x[n][p - 3 + r][q - 3 + s][c] * w[r][s][c]   (FLIP: w[K-1-r][K-1-s][c])
// grid.x = (row tile, column tile, channel group), channel group fastest; grid.y = image
template <int DT, int K, int TW, int CVB, bool FLIP, bool BIAS>
__global__ __launch_bounds__(256, 2) void dwconv7_tile_kernel(const uint16_t* __restrict__ x,
                                                              const uint16_t* __restrict__ w,
                                                              const uint16_t* __restrict__ bias,
                                                              uint16_t* __restrict__ y, int H, int W, int C, int G,
                                                              int TWN, FastDiv dG, FastDiv dTWN) {
  static_assert(TW * CVB == 256, "one thread per (column, channel vector)");
  constexpr int PAD = K / 2, TH = tile_th<TW>(), HR = TH + K - 1, HC = TW + K - 1;
  __shared__ uint4 halo[HR * HC * CVB];  // [halo row][halo column][channel vector]
  const int tid = threadIdx.x;
  const uint32_t t = fdiv(blockIdx.x, dG);
  const int cg = (int)(blockIdx.x - t * (uint32_t)G);
  const int th = (int)fdiv(t, dTWN);
  const int tw = (int)t - th * TWN;
  const int p0 = th * TH, q0 = tw * TW, cbase = cg * CVB * 8;
  const uint16_t* xn = x + (int64_t)blockIdx.y * H * W * C;

  for (int idx = tid; idx < HR * HC * CVB; idx += 256) {
    const int cv = idx % CVB, hc = (idx / CVB) % HC, hr = idx / (CVB * HC);
    const int ih = p0 - PAD + hr, iw = q0 - PAD + hc, c = cbase + cv * 8;
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (ih >= 0 && ih < H && iw >= 0 && iw < W && c < C) v = *(const uint4*)(xn + ((ih * W + iw) * C + c));
    halo[idx] = v;
  }
  __syncthreads();

  const int cvi = tid % CVB, col = tid / CVB;
  const int c0 = cbase + cvi * 8, q = q0 + col;
  if (c0 >= C || q >= W) return;  // after the only barrier

  float acc[TH][8];
#pragma unroll
  for (int i = 0; i < TH; ++i)
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[i][e] = 0.f;

#pragma unroll 1
  for (int s = 0; s < K; ++s) {
    float wf[K][8];
#pragma unroll
    for (int r = 0; r < K; ++r) {
      const int tap = FLIP ? K * K - 1 - (r * K + s) : r * K + s;
      unpack8f7<DT>(*(const uint4*)(w + (tap * C + c0)), wf[r]);
    }
    const uint4* hp = halo + (col + s) * CVB + cvi;
#pragma unroll
    for (int j = 0; j < HR; ++j) {
      float xf[8];
      unpack8f7<DT>(hp[j * HC * CVB], xf);
#pragma unroll
      for (int i = 0; i < TH; ++i) {
        const int r = j - i;
        if (r >= 0 && r < K) {
#pragma unroll
          for (int e = 0; e < 8; ++e) acc[i][e] += xf[e] * wf[r][e];
        }
      }
    }
  }

  float bf[8];
  if constexpr (BIAS) unpack8f7<DT>(*(const uint4*)(bias + c0), bf);
  uint16_t* yn = y + (int64_t)blockIdx.y * H * W * C;
#pragma unroll
  for (int i = 0; i < TH; ++i) {
    const int p = p0 + i;
    if constexpr (BIAS) {
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[i][e] += bf[e];
    }
    if (p < H) *(uint4*)(yn + ((p * W + q) * C + c0)) = pack8f7<DT>(acc[i]);
  }
}

// geometry of the weight-gradient block: 8 channel vectors x 8 row slots x 4 pixel lanes
constexpr int kWgCVB = 8;   // channel vectors per block
constexpr int kWgBR = 8;    // output rows per band: two per pixel lane
constexpr int kWgWC = 14;   // output columns per band: two trips of the 7-wide window (ConvNeXt's maps: 56 28 14 7)
constexpr int kWgMinPix = 128;  // fewest pixels a split is given (a split restages the halo of its partial rows)

// Partial slab ws[blockIdx.y][r * K + s][c] = sum over the block's pixel range [start, end) of
// x[n][p - 3 + r][q - 3 + s][c] * dy[n][p][q][c]; row K * K = the sum of dy.  The range is walked in bands of rows of
// one image; a pixel outside the range (the partial first and last rows) is masked where dy is staged: a zero dy
// adds nothing to either gradient.
template <int DT, int K>
__global__ __launch_bounds__(256, 2) void dwconv7_wgrad_kernel(const uint16_t* __restrict__ x,
                                                               const uint16_t* __restrict__ dy,
                                                               float* __restrict__ ws, int npix, int pps, int H,
                                                               int W, int C, FastDiv dW, FastDiv dH) {
  static_assert(K == 7, "8 row slots = 7 kernel rows + the bias slot");
  constexpr int PAD = K / 2, CVB = kWgCVB, BR = kWgBR, WC = kWgWC, HR = BR + K - 1, HC = WC + K - 1;
  // x rows are (HC + 1) * 128 bytes apart: an odd multiple of 128, so the 8 row slots of a lane group fall on
  // distinct banks (tools/lds_sim.py dwconv7; HC * 128 = 2560 is a multiple of 256 and conflicts 2-way)
  constexpr int XSV = (HC + 1) * CVB;
  // one row more than the halo: the bias slot reads "kernel row 7" (never staged, its value is replaced by 1.0), so
  // the 8 slots keep 8 distinct rows and the read stays conflict-free
  constexpr int XV = (HR + 1) * XSV, DV = BR * WC * CVB, RV = 256 * K * 8 / 4;  // in 16-byte vectors
  __shared__ uint4 smem[XV + DV > RV ? XV + DV : RV];  // staging, then the lane reduction
  uint4* xs = smem;
  uint4* ds = smem + XV;

  const int tid = threadIdx.x;
  const int cv = tid & 7, slot = (tid >> 3) & 7, lane = tid >> 6;
  const int r = slot;          // slot 7, the bias slot, replaces what it reads by 1.0: acc[0] becomes the sum of dy
  const bool ones = slot == K;
  const int cbase = blockIdx.x * CVB * 8;

  float acc[K][8];
#pragma unroll
  for (int s = 0; s < K; ++s)
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[s][e] = 0.f;

  const int start = blockIdx.y * pps;
  const int end = min(start + pps, npix);
  const int g0 = end > start ? (int)fdiv((uint32_t)start, dW) : 0;       // global rows n * H + p
  const int g1 = end > start ? (int)fdiv((uint32_t)(end - 1), dW) : -1;
  for (int g = g0; g <= g1;) {
    const int n = (int)fdiv((uint32_t)g, dH);
    const int p = g - n * H;
    const int rows = min(min(BR, H - p), g1 + 1 - g);  // a band stays inside one image
    const uint16_t* xn = x + (int64_t)n * H * W * C;
    for (int qc = 0; qc < W; qc += WC) {
      const int wc = min(WC, W - qc);
      __syncthreads();  // the previous band's reads are done
      for (int idx = tid; idx < HR * HC * CVB; idx += 256) {
        const int v = idx & 7, hc = (idx >> 3) % HC, hr = (idx >> 3) / HC;
        const int ih = p - PAD + hr, iw = qc - PAD + hc, c = cbase + v * 8;
        uint4 val = make_uint4(0u, 0u, 0u, 0u);
        if (hr < rows + K - 1 && ih >= 0 && ih < H && iw >= 0 && iw < W && c < C)
          val = *(const uint4*)(xn + ((ih * W + iw) * C + c));
        xs[hr * XSV + hc * CVB + v] = val;
      }
      for (int idx = tid; idx < DV; idx += 256) {
        const int v = idx & 7, dc = (idx >> 3) % WC, i = (idx >> 3) / WC;
        const int pix = (g + i) * W + qc + dc, c = cbase + v * 8;
        uint4 val = make_uint4(0u, 0u, 0u, 0u);
        if (i < rows && dc < wc && pix >= start && pix < end && c < C) val = *(const uint4*)(dy + ((int64_t)pix * C + c));
        ds[idx] = val;
      }
      __syncthreads();
      for (int i = lane; i < rows; i += 4) {
        const uint4* xr = xs + (i + r) * XSV + cv;
        const uint4* dr = ds + i * WC * CVB + cv;
        // xw[c % 7] holds halo column c; step q multiplies columns q .. q + 6 by dy[q]
        float xw[K][8];
#pragma unroll
        for (int c = 0; c < K - 1; ++c) {
          unpack8f7<DT>(xr[c * CVB], xw[c]);
          if (ones) {
#pragma unroll
            for (int e = 0; e < 8; ++e) xw[c][e] = 1.f;
          }
        }
#pragma unroll 1
        for (int qb = 0; qb < wc; qb += K) {
#pragma unroll
          for (int k = 0; k < K; ++k) {
            if (qb + k < wc) {  // uniform
              unpack8f7<DT>(xr[(qb + k + K - 1) * CVB], xw[(k + K - 1) % K]);
              if (ones) {
#pragma unroll
                for (int e = 0; e < 8; ++e) xw[(k + K - 1) % K][e] = 1.f;
              }
              float gf[8];
              unpack8f7<DT>(dr[(qb + k) * CVB], gf);
#pragma unroll
              for (int s = 0; s < K; ++s)
#pragma unroll
                for (int e = 0; e < 8; ++e) acc[s][e] += xw[(k + s) % K][e] * gf[e];
            }
          }
        }
      }
    }
    g += rows;
  }

  // red[tid][s][e], tid = (lane * 8 + slot) * 8 + cv
  __syncthreads();
  float* red = (float*)smem;
#pragma unroll
  for (int s = 0; s < K; ++s) {
    *(f32x4_t*)&red[(tid * K + s) * 8] = f32x4_t{acc[s][0], acc[s][1], acc[s][2], acc[s][3]};
    *(f32x4_t*)&red[(tid * K + s) * 8 + 4] = f32x4_t{acc[s][4], acc[s][5], acc[s][6], acc[s][7]};
  }
  __syncthreads();
  float* slab = ws + (int64_t)blockIdx.y * (K * K + 1) * C;
  for (int o = tid; o < (K * K + 1) * CVB * 8; o += 256) {
    const int e = o & 7, ci = (o >> 3) & 7, row = o >> 6;
    const int c = cbase + ci * 8 + e;
    if (c >= C) continue;
    const int rr = row < K * K ? row / K : K, ss = row < K * K ? row - rr * K : 0;  // row 49: the bias slot's s = 0
    float sum = 0.f;
#pragma unroll
    for (int l = 0; l < 4; ++l) sum += red[((((l * 8 + rr) * 8 + ci) * K) + ss) * 8 + e];
    slab[(int64_t)row * C + c] = sum;
  }
}

template <int DT, bool FLIP, bool BIAS>
void tile_launch(const uint16_t* x, const uint16_t* w, const uint16_t* bias, uint16_t* y, int64_t N, int H, int W,
                 int C, hipStream_t s) {
  // the tile width from W alone: the narrowest of 8 / 16 / 32 columns that holds the row, 32 beyond that
  const int TW = W <= 8 ? 8 : (W <= 16 ? 16 : 32);
  const int CVB = 256 / TW, TH = TW == 8 ? tile_th<8>() : tile_th<32>();
  const int G = (C / 8 + CVB - 1) / CVB, TWN = (W + TW - 1) / TW, THN = (H + TH - 1) / TH;
  const int64_t blocks = (int64_t)G * TWN * THN;
  if (blocks >= (int64_t(1) << 31))
    pdt_hip_fail("dwconv7_tile: more than 2^31 tiles per image", hipErrorInvalidValue, __FILE__, __LINE__);
  const dim3 g((unsigned)blocks, (unsigned)N);
  const FastDiv dG = make_fastdiv((uint32_t)G), dTWN = make_fastdiv((uint32_t)TWN);
#define PDT_DW7_T(TWv, CVBv)                                                                                       \
  hipLaunchKernelGGL((dwconv7_tile_kernel<DT, 7, TWv, CVBv, FLIP, BIAS>), g, dim3(256), 0, s, x, w, bias, y, H, W, \
                     C, G, TWN, dG, dTWN)
  if (TW == 32) PDT_DW7_T(32, 8);
  else if (TW == 16) PDT_DW7_T(16, 16);
  else if (TW == 8) PDT_DW7_T(8, 32);
  else pdt_hip_fail("dwconv7_tile: no instantiation for this width", hipErrorInvalidValue, __FILE__, __LINE__);
#undef PDT_DW7_T
}

void check_geom(const char* what, int dtype, int64_t N, int H, int W, int C) {
  if ((dtype != kBF16 && dtype != kF16) || N < 0 || N > 65535 || H <= 0 || W <= 0 || C <= 0 || C % 8 != 0 ||
      (int64_t)H * W * C >= (int64_t(1) << 31))
    pdt_hip_fail(what, hipErrorInvalidValue, __FILE__, __LINE__);
}

}  // namespace

void dwconv7_fwd_launch(int dtype, const uint16_t* x, const uint16_t* w, const uint16_t* bias, uint16_t* y, int64_t N,
                        int H, int W, int C, hipStream_t s) {
  check_geom("dwconv7_fwd_launch: geometry outside the kernels' contract", dtype, N, H, W, C);
  if (N == 0) return;
  PDT_COUNT("dwconv7_fwd");
  if (dtype == kBF16) {
    if (bias) tile_launch<kBF16, false, true>(x, w, bias, y, N, H, W, C, s);
    else tile_launch<kBF16, false, false>(x, w, bias, y, N, H, W, C, s);
  } else {
    if (bias) tile_launch<kF16, false, true>(x, w, bias, y, N, H, W, C, s);
    else tile_launch<kF16, false, false>(x, w, bias, y, N, H, W, C, s);
  }
}

void dwconv7_dgrad_launch(int dtype, const uint16_t* dy, const uint16_t* w, uint16_t* dx, int64_t N, int H, int W,
                          int C, hipStream_t s) {
  check_geom("dwconv7_dgrad_launch: geometry outside the kernels' contract", dtype, N, H, W, C);
  if (N == 0) return;
  PDT_COUNT("dwconv7_dgrad");
  if (dtype == kBF16) tile_launch<kBF16, true, false>(dy, w, nullptr, dx, N, H, W, C, s);
  else tile_launch<kF16, true, false>(dy, w, nullptr, dx, N, H, W, C, s);
}

Dw7WgradPlan dwconv7_wgrad_plan(int64_t npix, int C, int target_blocks) {
  Dw7WgradPlan pl{};
  pl.groups = (C / 8 + kWgCVB - 1) / kWgCVB;
  if (pl.groups < 1) pl.groups = 1;
  int64_t splits = ((int64_t)target_blocks + pl.groups - 1) / pl.groups;
  const int64_t most = (npix + kWgMinPix - 1) / kWgMinPix;
  if (splits > most) splits = most;
  if (splits > 65535) splits = 65535;  // grid.y
  if (splits < 1) splits = 1;
  const int64_t pps = npix > 0 ? (npix + splits - 1) / splits : 1;
  pl.pix_per_split = (int)pps;
  pl.splits = npix > 0 ? (int)((npix + pps - 1) / pps) : 1;
  return pl;
}

void dwconv7_wgrad_launch(int dtype, const uint16_t* x, const uint16_t* dy, float* ws, int64_t N, int H, int W, int C,
                          const Dw7WgradPlan& plan, hipStream_t s) {
  check_geom("dwconv7_wgrad_launch: geometry outside the kernels' contract", dtype, N, H, W, C);
  const int64_t npix = N * H * W;
  if (npix <= 0 || npix >= (int64_t(1) << 30) || plan.splits < 1 || plan.splits > 65535 || plan.pix_per_split < 1 ||
      (int64_t)plan.splits * plan.pix_per_split < npix || plan.groups != (C / 8 + kWgCVB - 1) / kWgCVB)
    pdt_hip_fail("dwconv7_wgrad_launch: the plan does not cover the pixels", hipErrorInvalidValue, __FILE__, __LINE__);
  PDT_COUNT("dwconv7_wgrad");
  const dim3 g((unsigned)plan.groups, (unsigned)plan.splits);
  const FastDiv dW = make_fastdiv((uint32_t)W), dH = make_fastdiv((uint32_t)H);
  if (dtype == kBF16)
    hipLaunchKernelGGL((dwconv7_wgrad_kernel<kBF16, 7>), g, dim3(256), 0, s, x, dy, ws, (int)npix, plan.pix_per_split,
                       H, W, C, dW, dH);
  else
    hipLaunchKernelGGL((dwconv7_wgrad_kernel<kF16, 7>), g, dim3(256), 0, s, x, dy, ws, (int)npix, plan.pix_per_split,
                       H, W, C, dW, dH);
}

}  // namespace pdt
