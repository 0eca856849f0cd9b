// Depthwise convolution kernels (SURVEY §2.2 model registry: MobileNetV2/V3, MNASNet, EfficientNet, ShuffleNetV2):
// groups == Cin == Cout == C, square kernel R = S in {3, 5}, stride in {1, 2}, dilation 1, pad R / 2, C % 8 == 0.
// NHWC 16-bit activations, taps-major [R][S][C] 16-bit weight (one tap's 8 channels = one 16-byte load), fp32 math,
// 64-bit element offsets (MobileNetV2's 112 x 112 x 96 activation passes 2^31 elements at a few hundred images).
// VALU / bandwidth bound: no MFMA, no LDS on the activation path.  A thread owns 8 channels (one 16-byte vector);
// consecutive lanes take consecutive channel vectors, then consecutive pixels, so a wave's accesses are contiguous.
//   * dwconv_strip: forward (and the stride-1 backward data, which is the same conv with the taps flipped).  A
//     thread computes a column strip of TH output rows: each input row's S vectors are loaded once and feed every
//     output row of the strip they touch (vertical reuse in registers; horizontal reuse between neighbouring
//     lanes through L1 / L2).
//   * dwconv_dgrad2: stride-2 backward data in gather form.  A thread owns a 2 x 2 dx quad = all four sub-pixel
//     phases off one shared dy window, so the tap selection is compile-time and uniform (no parity branch), and
//     every dx element is written exactly once.
//   * dwconv_wgrad: a block reduces its pixel range for `cvb` channel vectors; the kernel rows are split over
//     threads (S * 8 accumulators each, 200 would not fit for 5 x 5), pixel lanes are summed through LDS in a
//     fixed order and the block writes one partial slab [split][R * S][C] for wgrad_reduce (no float atomics).
#include "../common.h"
#include "dwconv.h"

namespace pdt {

namespace {

template <int DT>
PDT_DEVICE void unpack8f(uint4 v, float (&o)[8]) {
  uint16_t h[8];
  unpack8(v, h);
#pragma unroll
  for (int e = 0; e < 8; ++e) o[e] = E16<DT>::to_f(h[e]);
}

template <int DT>
PDT_DEVICE uint4 pack8f(const float (&a)[8]) {
  using E = E16<DT>;
  return make_uint4(E::pack2(a[0], a[1]), E::pack2(a[2], a[3]), E::pack2(a[4], a[5]), E::pack2(a[6], a[7]));
}

// element e of a packed 8 x 16-bit vector as fp32
template <int DT>
PDT_DEVICE float elem_f(const uint4& v, int e) {
  const uint32_t w = e < 2 ? v.x : e < 4 ? v.y : e < 6 ? v.z : v.w;
  return E16<DT>::to_f((uint16_t)(w >> (16 * (e & 1))));
}

// 16-byte load that is zero where !ok: the caller passes an address that is valid either way (clamped into the
// tensor), so the load is unconditional and the code stays one basic block (a branch per tap defeats the scheduler)
PDT_DEVICE uint4 ld16_or_zero(const uint16_t* p, bool ok) {
  const uint4 v = *(const uint4*)p;
  return make_uint4(ok ? v.x : 0u, ok ? v.y : 0u, ok ? v.z : 0u, ok ? v.w : 0u);
}

PDT_DEVICE int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// Output rows per thread of dwconv_strip.  A tap that serves more than one output row is kept expanded to fp32 by
// the compiler (R * S * 8 VGPRs: 72 for 3 x 3, 200 for 5 x 5 -- more than the budget), so 3 x 3 strips are 4 rows
// high (measured against 1 and 2: profiles/dwconv_mi355x.md) and a 5 x 5 thread computes one row, converting its
// packed weights (100 VGPRs) at their single use.
template <int R> constexpr int strip_th() { return R == 3 ? 4 : 1; }

// y[n][p][q][c] = sum_{r,s} x[n][p*ST - PAD + r][q*ST - PAD + s][c] * w[r][s][c]   (FLIP: w[R-1-r][S-1-s][c])
template <int DT, int R, int ST, bool FLIP>
__global__ __launch_bounds__(256) void dwconv_strip_kernel(const uint16_t* __restrict__ x,
                                                           const uint16_t* __restrict__ w,
                                                           uint16_t* __restrict__ y, uint32_t per_img, int H,
                                                           int W, int C, int P, int Q, FastDiv dCV, FastDiv dQ) {
  constexpr int S = R, PAD = R / 2, TH = strip_th<R>(), ROWS = ST * (TH - 1) + R;
  // blockIdx.y = image: the image base is wave-uniform 64-bit, everything inside an image is 32-bit
  const uint32_t v = blockIdx.x * 256u + threadIdx.x;
  if (v >= per_img) return;
  const uint32_t t = fdiv(v, dCV);
  const int c0 = (int)(v - t * (uint32_t)(C / 8)) * 8;
  const uint32_t ps = fdiv(t, dQ);
  const int q = (int)(t - ps * (uint32_t)Q);
  const int p0 = (int)ps * TH;

  uint4 wp[R * S];
#pragma unroll
  for (int k = 0; k < R * S; ++k) wp[k] = *(const uint4*)(w + (int64_t)(FLIP ? R * S - 1 - k : k) * C + c0);

  float acc[TH][8];
#pragma unroll
  for (int i = 0; i < TH; ++i)
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[i][e] = 0.f;

  const int ih0 = p0 * ST - PAD, iw0 = q * ST - PAD;
  const uint16_t* xn = x + (int64_t)blockIdx.y * H * W * C;
  uint16_t* yn = y + (int64_t)blockIdx.y * P * Q * C;
  // every load of the strip is independent of the arithmetic, so the compiler issues all ROWS * S of them up front
  // (ROWS * S * 4 VGPRs): with two waves per SIMD the kernel lives on the loads each wave keeps in flight
#pragma unroll
  for (int j = 0; j < ROWS; ++j) {
    const int ih = ih0 + j;
    const bool rok = ih >= 0 && ih < H;
#pragma unroll
    for (int s = 0; s < S; ++s) {
      const int iw = iw0 + s;
      const uint4 xv =
          ld16_or_zero(xn + ((clampi(ih, H - 1) * W + clampi(iw, W - 1)) * C + c0), rok && iw >= 0 && iw < W);
      float xf[8];
      unpack8f<DT>(xv, xf);
#pragma unroll
      for (int i = 0; i < TH; ++i) {
        const int r = j - ST * i;
        if (r >= 0 && r < R) {
#pragma unroll
          for (int e = 0; e < 8; ++e) acc[i][e] += xf[e] * elem_f<DT>(wp[r * S + s], e);
        }
      }
    }
  }
#pragma unroll
  for (int i = 0; i < TH; ++i) {
    const int p = p0 + i;
    if (p < P) *(uint4*)(yn + ((p * Q + q) * C + c0)) = pack8f<DT>(acc[i]);
  }
}

// dx[n][2i+a][2j+b][c] = sum over the taps r = a + PAD - 2*dp, s = b + PAD - 2*dq of dy[n][i+dp][j+dq][c] * w[r][s][c]
// for the dy window dp, dq in [DLO, DHI] (2 x 2 for 3 x 3, 3 x 3 for 5 x 5): each tap belongs to exactly one phase.
template <int DT, int R>
__global__ __launch_bounds__(256) void dwconv_dgrad2_kernel(const uint16_t* __restrict__ dy,
                                                            const uint16_t* __restrict__ w,
                                                            uint16_t* __restrict__ dx, uint32_t per_img, int H,
                                                            int W, int C, int P, int Q, FastDiv dCV, FastDiv dWQ,
                                                            int WQ) {
  constexpr int S = R, PAD = R / 2, DLO = -((R - 1 - PAD) / 2), DHI = (1 + PAD) / 2, NW = DHI - DLO + 1;
  const uint32_t v = blockIdx.x * 256u + threadIdx.x;
  if (v >= per_img) return;
  const uint32_t t = fdiv(v, dCV);
  const int c0 = (int)(v - t * (uint32_t)(C / 8)) * 8;
  const int i = (int)fdiv(t, dWQ);
  const int j = (int)t - i * WQ;

  uint4 wp[R * S];
#pragma unroll
  for (int k = 0; k < R * S; ++k) wp[k] = *(const uint4*)(w + (int64_t)k * C + c0);

  float acc[2][2][8];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[a][b][e] = 0.f;

  const uint16_t* dyn = dy + (int64_t)blockIdx.y * P * Q * C;
  uint16_t* dxn = dx + (int64_t)blockIdx.y * H * W * C;
#pragma unroll
  for (int u = 0; u < NW; ++u) {
    const int p = i + DLO + u;
    const bool rok = p >= 0 && p < P;
#pragma unroll
    for (int z = 0; z < NW; ++z) {
      const int q = j + DLO + z;
      const uint4 gv = ld16_or_zero(dyn + ((clampi(p, P - 1) * Q + clampi(q, Q - 1)) * C + c0), rok && q >= 0 && q < Q);
      float gf[8];
      unpack8f<DT>(gv, gf);
#pragma unroll
      for (int a = 0; a < 2; ++a) {
        const int r = a + PAD - 2 * (DLO + u);
        if (r < 0 || r >= R) continue;
#pragma unroll
        for (int b = 0; b < 2; ++b) {
          const int s = b + PAD - 2 * (DLO + z);
          if (s < 0 || s >= S) continue;
#pragma unroll
          for (int e = 0; e < 8; ++e) acc[a][b][e] += gf[e] * elem_f<DT>(wp[r * S + s], e);
        }
      }
    }
  }
#pragma unroll
  for (int a = 0; a < 2; ++a) {
    const int h = 2 * i + a;
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      const int ww = 2 * j + b;
      if (h < H && ww < W) *(uint4*)(dxn + ((h * W + ww) * C + c0)) = pack8f<DT>(acc[a][b]);
    }
  }
}

// Partial slab ws[blockIdx.y][r*S + s][c] = sum over the block's pixel range of x[n][p*ST-PAD+r][q*ST-PAD+s][c] *
// dy[n][p][q][c].  Thread = (channel vector cvi, pixel lane pl, kernel row r), cvi fastest: a wave reads contiguous
// channel vectors of consecutive pixels of (mostly) one kernel row.  Fixed summation order: a lane walks its pixels
// in order, then the pixel lanes are added in lane order.
template <int DT, int R, int ST>
__global__ __launch_bounds__(256) void dwconv_wgrad_kernel(const uint16_t* __restrict__ x,
                                                           const uint16_t* __restrict__ dy, float* __restrict__ ws,
                                                           int npix, int pps, int H, int W, int C, int P, int Q,
                                                           FastDiv dQ, FastDiv dP, int CVB, int PL) {
  constexpr int S = R, PAD = R / 2;
  __shared__ float red[256 * S * 8];
  const int tid = threadIdx.x;
  const int cvi = tid % CVB;
  const int pl = (tid / CVB) % PL;
  const int r = tid / (CVB * PL);
  const int c0 = (blockIdx.x * CVB + cvi) * 8;
  float acc[S][8];
#pragma unroll
  for (int s = 0; s < S; ++s)
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[s][e] = 0.f;

  if (r < R && c0 < C) {
    const int start = blockIdx.y * pps;
    const int end = min(start + pps, npix);
    // UN pixels per trip, branch-free (a pixel past the range or a padding row / column loads a clamped address and
    // is zeroed), so their loads are all in flight before the first FMA
    constexpr int UN = R == 3 ? 4 : 2;
    for (int pix0 = start + pl; pix0 < end; pix0 += PL * UN) {
      uint4 gv[UN], xv[UN][S];
#pragma unroll
      for (int k = 0; k < UN; ++k) {
        const bool pok = pix0 + k * PL < end;
        const int pix = pok ? pix0 + k * PL : end - 1;
        const uint32_t t = fdiv((uint32_t)pix, dQ);
        const int q = pix - (int)t * Q;
        const uint32_t n = fdiv(t, dP);
        const int p = (int)t - (int)n * P;
        const int ih = p * ST - PAD + r;
        const bool rok = pok && ih >= 0 && ih < H;
        gv[k] = ld16_or_zero(dy + (int64_t)pix * C + c0, rok);
        const uint16_t* xr = x + ((int64_t)n * H + clampi(ih, H - 1)) * W * C + c0;
        const int iw0 = q * ST - PAD;
#pragma unroll
        for (int s = 0; s < S; ++s) {
          const int iw = iw0 + s;
          xv[k][s] = ld16_or_zero(xr + (int64_t)clampi(iw, W - 1) * C, rok && iw >= 0 && iw < W);
        }
      }
#pragma unroll
      for (int k = 0; k < UN; ++k) {
        float gf[8];
        unpack8f<DT>(gv[k], gf);
#pragma unroll
        for (int s = 0; s < S; ++s) {
          float xf[8];
          unpack8f<DT>(xv[k][s], xf);
#pragma unroll
          for (int e = 0; e < 8; ++e) acc[s][e] += xf[e] * gf[e];
        }
      }
    }
  }
  // red[tid][s][e], tid = (r * PL + pl) * CVB + cvi
#pragma unroll
  for (int s = 0; s < S; ++s) {
    *(f32x4_t*)&red[(tid * S + s) * 8] = f32x4_t{acc[s][0], acc[s][1], acc[s][2], acc[s][3]};
    *(f32x4_t*)&red[(tid * S + s) * 8 + 4] = f32x4_t{acc[s][4], acc[s][5], acc[s][6], acc[s][7]};
  }
  __syncthreads();
  float* slab = ws + (int64_t)blockIdx.y * (R * S) * C;
  const int nout = R * S * CVB * 8;  // (r, s, cvi, e)
  for (int o = tid; o < nout; o += 256) {
    const int e = o & 7;
    const int ci = (o >> 3) % CVB;
    const int rs = (o >> 3) / CVB;
    const int rr = rs / S, ss = rs - rr * S;
    const int c = (blockIdx.x * CVB + ci) * 8 + e;
    if (c >= C) continue;
    float sum = 0.f;
    for (int l = 0; l < PL; ++l) sum += red[(((rr * PL + l) * CVB + ci) * S + ss) * 8 + e];
    slab[(int64_t)rs * C + c] = sum;
  }
}

// grid = (blocks over one image's work items, images); the bindings check N <= 65535 and H * W * C < 2^31
dim3 dw_grid(int64_t per_img, int64_t N) { return dim3((unsigned)((per_img + 255) / 256), (unsigned)N); }

}  // namespace

void dwconv_fwd_launch(int dtype, const uint16_t* x, const uint16_t* w, uint16_t* y, int64_t N, int H, int W, int C,
                       int R, int stride, hipStream_t s) {
  const int TH = R == 3 ? strip_th<3>() : strip_th<5>();
  const int P = (H - 1) / stride + 1, Q = (W - 1) / stride + 1, PS = (P + TH - 1) / TH;
  const int64_t per_img = (int64_t)PS * Q * (C / 8);
  if (N * per_img == 0) return;
  const FastDiv dCV = make_fastdiv((uint32_t)(C / 8)), dQ = make_fastdiv((uint32_t)Q);
  PDT_COUNT("dwconv_fwd");
#define PDT_DW_F(DT, RR, ST)                                                                                      \
  hipLaunchKernelGGL((dwconv_strip_kernel<DT, RR, ST, false>), dw_grid(per_img, N), dim3(256), 0, s, x, w, y,    \
                     (uint32_t)per_img, H, W, C, P, Q, dCV, dQ)
#define PDT_DW_F2(DT)                                     \
  do {                                                    \
    if (R == 3 && stride == 1) PDT_DW_F(DT, 3, 1);        \
    else if (R == 3) PDT_DW_F(DT, 3, 2);                  \
    else if (stride == 1) PDT_DW_F(DT, 5, 1);             \
    else PDT_DW_F(DT, 5, 2);                              \
  } while (0)
  if (dtype == kBF16) PDT_DW_F2(kBF16); else PDT_DW_F2(kF16);
#undef PDT_DW_F2
#undef PDT_DW_F
}

void dwconv_dgrad_launch(int dtype, const uint16_t* dy, const uint16_t* w, uint16_t* dx, int64_t N, int H, int W,
                         int C, int R, int stride, hipStream_t s) {
  const int P = (H - 1) / stride + 1, Q = (W - 1) / stride + 1;
  if (N * H * W * C == 0) return;
  const FastDiv dCV = make_fastdiv((uint32_t)(C / 8));
  PDT_COUNT("dwconv_dgrad");
  if (stride == 1) {
    // the same conv over dy (P == H, Q == W) with the taps flipped
    const int TH = R == 3 ? strip_th<3>() : strip_th<5>();
    const int PS = (H + TH - 1) / TH;
    const int64_t per_img = (int64_t)PS * W * (C / 8);
    const FastDiv dQ = make_fastdiv((uint32_t)W);
#define PDT_DW_D1(DT, RR)                                                                                         \
  hipLaunchKernelGGL((dwconv_strip_kernel<DT, RR, 1, true>), dw_grid(per_img, N), dim3(256), 0, s, dy, w, dx,     \
                     (uint32_t)per_img, H, W, C, H, W, dCV, dQ)
    if (dtype == kBF16) { if (R == 3) PDT_DW_D1(kBF16, 3); else PDT_DW_D1(kBF16, 5); }
    else { if (R == 3) PDT_DW_D1(kF16, 3); else PDT_DW_D1(kF16, 5); }
#undef PDT_DW_D1
  } else {
    const int HQ = (H + 1) / 2, WQ = (W + 1) / 2;
    const int64_t per_img = (int64_t)HQ * WQ * (C / 8);
    const FastDiv dWQ = make_fastdiv((uint32_t)WQ);
#define PDT_DW_D2(DT, RR)                                                                                         \
  hipLaunchKernelGGL((dwconv_dgrad2_kernel<DT, RR>), dw_grid(per_img, N), dim3(256), 0, s, dy, w, dx,             \
                     (uint32_t)per_img, H, W, C, P, Q, dCV, dWQ, WQ)
    if (dtype == kBF16) { if (R == 3) PDT_DW_D2(kBF16, 3); else PDT_DW_D2(kBF16, 5); }
    else { if (R == 3) PDT_DW_D2(kF16, 3); else PDT_DW_D2(kF16, 5); }
#undef PDT_DW_D2
  }
}

DwWgradPlan dwconv_wgrad_plan(int64_t npix, int C, int R, int target_blocks) {
  DwWgradPlan pl{};
  const int cv = C / 8;
  // 4 .. 8 vectors (64 .. 128 contiguous bytes per pixel) per block: the count that pads the channels least, the
  // larger on a tie (18 vectors: 3 groups of 6, not 8 + 8 + 2)
  pl.cvb = cv < 8 ? cv : 8;
  if (cv > 8) {
    int waste = (cv + 7) / 8 * 8 - cv;
    for (int b = 7; b >= 4; --b) {
      const int wb = (cv + b - 1) / b * b - cv;
      if (wb < waste) { waste = wb; pl.cvb = b; }
    }
  }
  pl.pl = 256 / (pl.cvb * R);
  pl.groups = (cv + pl.cvb - 1) / pl.cvb;
  if (pl.groups < 1) pl.groups = 1;
  int64_t splits = ((int64_t)target_blocks + pl.groups - 1) / pl.groups;
  const int64_t most = (npix + pl.pl - 1) / pl.pl;  // at least one pixel per lane
  if (splits > most) splits = most;
  if (splits > 65535) splits = 65535;  // grid.y
  if (splits < 1) splits = 1;
  const int64_t pps = npix > 0 ? (npix + splits - 1) / splits : 1;
  pl.pix_per_split = (int)pps;
  pl.splits = npix > 0 ? (int)((npix + pps - 1) / pps) : 1;
  return pl;
}

void dwconv_wgrad_launch(int dtype, const uint16_t* x, const uint16_t* dy, float* ws, int64_t N, int H, int W, int C,
                         int R, int stride, const DwWgradPlan& plan, hipStream_t s) {
  const int P = (H - 1) / stride + 1, Q = (W - 1) / stride + 1;
  const int npix = (int)(N * P * Q);  // < 2^31 (checked by the binding): FastDiv dividends
  PDT_COUNT("dwconv_wgrad");
  const dim3 g((unsigned)plan.groups, (unsigned)plan.splits);
  const FastDiv dQ = make_fastdiv((uint32_t)Q), dP = make_fastdiv((uint32_t)P);
#define PDT_DW_W(DT, RR, ST)                                                                                      \
  hipLaunchKernelGGL((dwconv_wgrad_kernel<DT, RR, ST>), g, dim3(256), 0, s, x, dy, ws, npix, plan.pix_per_split,  \
                     H, W, C, P, Q, dQ, dP, plan.cvb, plan.pl)
#define PDT_DW_W2(DT)                                     \
  do {                                                    \
    if (R == 3 && stride == 1) PDT_DW_W(DT, 3, 1);        \
    else if (R == 3) PDT_DW_W(DT, 3, 2);                  \
    else if (stride == 1) PDT_DW_W(DT, 5, 1);             \
    else PDT_DW_W(DT, 5, 2);                              \
  } while (0)
  if (dtype == kBF16) PDT_DW_W2(kBF16); else PDT_DW_W2(kF16);
#undef PDT_DW_W2
#undef PDT_DW_W
}

}  // namespace pdt
