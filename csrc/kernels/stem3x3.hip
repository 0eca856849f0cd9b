// First conv of the depthwise-separable family (MobileNetV2/V3, MNASNet, EfficientNet, ShuffleNetV2): 3x3, stride 2,
// padding 1, 3 -> K channels (K % 8 == 0, 8 <= K <= 64), no bias, on the fp32 NHWC image the torch engine holds (the
// storage of a channels_last [N, 3, H, W] tensor: 12-byte pixels, 4-byte alignment).  No padded or 16-bit copy of the
// image is made: the patch matrix patch[m][j], j = (r * 3 + s) * 3 + c (27 terms, one 32-element MFMA K-step), is
// gathered from the image where it lies, rounded to the compute dtype to nearest even in registers (the value
// x.to(dtype) has) and fed to v_mfma_f32_16x16x32_{bf16,f16}; fp32 accumulation, wave64.
//
//   * stem_load8 / stem_pack8: the 8 reduction elements j = 8 * chunk + [0, 8) of one output pixel.  Within kernel row
//     r the 9 values (s, c) are 9 consecutive floats of input row 2p - 1 + r from column 2q - 1 on, so an element is
//     image[base(p, q) + r * 3W + 3s + c].  Padding (row / column -1, and H / W when the side is odd), the slots
//     27..31 and pixels past M are never read: their index is clamped to element 0 of the image and the loaded value
//     is replaced by +0, so no stale or neighbouring value ever meets a zero weight.  Neighbouring lanes read
//     neighbouring pixels (24 bytes apart): every cache line is used by the lanes of one or two instructions.
//   * stem3x3_fwd_kernel: y[m][k] = sum_j patch[m][j] * w[k][j].  The weights are the MFMA A operand with the
//     fragment-row permutation of conv1x1.hip / pwconv.hip, so a lane ends with 8 consecutive output channels of its
//     pixel: one 16-byte store, dropped past M or K (K = 8 mod 16 leaves the last row block half used).  The weight
//     fragments (at most 64 x 32 values, zeros past K and past j = 26) stay in registers for the block's life; a
//     block (4 waves) walks 256-pixel tiles of the flattened pixel index persistently, so a tile crosses output rows
//     and images freely (every pixel finds its own image base, 64-bit).
//   * stem3x3_wgrad_kernel: dw[k][j] = sum_m dy[m][k] * patch[m][j], the pixel index is the reduction: 128-pixel
//     steps of dy [pixel][64 ch] and of the patch [pixel][32] go through registers into a double-buffered LDS image
//     and are read back with ds_read_b64_tr_b16 (pwconv.hip's image and swizzle); two register sets keep the loads of
//     the next two steps in flight (a step has 8 MFMAs per wave: the loop waits on memory).  32 (j) x 64 (k) accumulator per
//     wave, each wave taking 32 pixels of a step; the waves are summed through LDS in a fixed order and the block
//     writes its split's slab [K][32] for wgrad_reduce (no atomics: bit-identical runs).
#include "../common.h"
#include "stem3x3.h"

namespace pdt {

namespace {

typedef unsigned int st_v4u __attribute__((vector_size(16)));
typedef __attribute__((address_space(3))) s16x4_t st_lds_s16x4;

PDT_DEVICE uint4 st_load16(__amdgpu_buffer_rsrc_t r, uint32_t off) {
  return __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(r, (int)off, 0, 0));
}

// output channel of row `row` of weight fragment i: fragments 2p and 2p + 1 give a lane (rows 4 * fq + r) the 8
// consecutive channels p * 32 + 8 * fq + [0, 8) (pwconv.hip's permutation)
PDT_DEVICE int st_frag_ch(int i, int row) { return (i >> 1) * 32 + (row >> 2) * 8 + (i & 1) * 4 + (row & 3); }

// The lane-constant description of reduction chunk `chunk`: element i is j = 8 * chunk + i = (r * 3 + s) * 3 + c;
// rel = offset (floats) from the window's first element, dr / ds = its kernel row / column.  A slot past the 27
// real terms gets a row far above the image: it fails the row test like padding does.
struct StemTaps {
  int rel[8], dr[8], ds[8];
};
PDT_DEVICE StemTaps stem_taps(int chunk, int W) {
  StemTaps t;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int j = chunk * 8 + i;
    const int r = j / 9, o = j - r * 9;
    t.rel[i] = r * W * 3 + o;
    t.dr[i] = j < kStemRed ? r : -(1 << 30);
    t.ds[i] = o / 3;
  }
  return t;
}

// output pixel m -> its image and the top-left input coordinate of its window
struct StemPix {
  const float* img;
  int ih0, iw0;
};
PDT_DEVICE StemPix stem_pixel(const float* x, uint32_t m, bool live, int H, int W, int P, int Q, FastDiv dQ,
                              FastDiv dP) {
  const uint32_t np = fdiv(m, dQ), q = m - np * (uint32_t)Q;
  const uint32_t n = fdiv(np, dP), p = np - n * (uint32_t)P;
  StemPix px;
  px.img = live ? x + (int64_t)n * ((int64_t)H * W * 3) : x;  // a pixel past M reads nothing: any valid base will do
  px.ih0 = 2 * (int)p - 1;
  px.iw0 = 2 * (int)q - 1;
  return px;
}

// raw fp32 values of one chunk and the mask of the elements that exist; every address is inside the pixel's image
PDT_DEVICE uint32_t stem_load8(const StemPix& px, bool live, int H, int W, const StemTaps& t, float (&v)[8]) {
  const int base = (px.ih0 * W + px.iw0) * 3;
  uint32_t mask = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const bool ok = live && (uint32_t)(px.ih0 + t.dr[i]) < (uint32_t)H && (uint32_t)(px.iw0 + t.ds[i]) < (uint32_t)W;
    v[i] = px.img[ok ? base + t.rel[i] : 0];
    mask |= ok ? (1u << i) : 0u;
  }
  return mask;
}

// rounded to nearest even and packed (element 2i in the low half of dword i); masked elements are +0
template <int DT>
PDT_DEVICE uint4 stem_pack8(const float (&v)[8], uint32_t mask) {
  using E = E16<DT>;
  uint32_t w[4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
    w[i] = E::pack2((mask >> (2 * i)) & 1 ? v[2 * i] : 0.f, (mask >> (2 * i + 1)) & 1 ? v[2 * i + 1] : 0.f);
  return make_uint4(w[0], w[1], w[2], w[3]);
}

template <int DT, int NG, int PT>
__global__ __launch_bounds__(256) void stem3x3_fwd_kernel(const float* __restrict__ x, const uint16_t* __restrict__ w,
                                                          uint16_t* __restrict__ y, int M, int H, int W, int K, int P,
                                                          int Q, FastDiv dQ, FastDiv dP, int mtiles) {
  using E = E16<DT>;
  typedef typename E::vec8 vec8;
  constexpr int NF = NG * 2;   // 16-channel weight fragments
  constexpr int WR = PT * 16;  // pixels per wave
  constexpr int BR = 4 * WR;   // pixels per block tile
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int fr = lane & 15, fq = lane >> 4;
  const StemTaps taps = stem_taps(fq, W);

  // weight fragments: row st_frag_ch(i, fr), reduction chunk fq; zeros past K and past the 27 real terms
  vec8 ares[NF];
#pragma unroll
  for (int i = 0; i < NF; ++i) {
    const int ch = st_frag_ch(i, fr);
    uint32_t pk[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int j = fq * 8 + e;
      const bool ok = ch < K && j < kStemRed;
      const uint32_t v = ok ? (uint32_t)w[ok ? ch * kStemRed + j : 0] : 0u;
      pk[e >> 1] |= v << ((e & 1) * 16);
    }
    ares[i] = __builtin_bit_cast(vec8, make_uint4(pk[0], pk[1], pk[2], pk[3]));
  }

  for (int t = blockIdx.x; t < mtiles; t += gridDim.x) {
    const int m0 = t * BR;  // < 2^30 + BR
    vec8 bf[PT];
#pragma unroll
    for (int j = 0; j < PT; ++j) {
      const int m = m0 + wave * WR + j * 16 + fr;
      const bool live = m < M;
      const StemPix px = stem_pixel(x, (uint32_t)m, live, H, W, P, Q, dQ, dP);
      float v[8];
      const uint32_t mask = stem_load8(px, live, H, W, taps, v);
      bf[j] = __builtin_bit_cast(vec8, stem_pack8<DT>(v, mask));
    }
    f32x4_t acc[NF][PT];
#pragma unroll
    for (int i = 0; i < NF; ++i)
#pragma unroll
      for (int j = 0; j < PT; ++j) acc[i][j] = E::mfma16x16x32(ares[i], bf[j], f32x4_t{0.f, 0.f, 0.f, 0.f});

    // fragment pair g gives the lane channels g * 32 + 8 * fq + [0, 8) of pixel m0 + wave * WR + j * 16 + fr
#pragma unroll
    for (int j = 0; j < PT; ++j) {
      const int m = m0 + wave * WR + j * 16 + fr;
#pragma unroll
      for (int g = 0; g < NG; ++g) {
        const int ch = g * 32 + 8 * fq;
        uint4 pk;
        pk.x = E::pack2(acc[2 * g][j][0], acc[2 * g][j][1]);
        pk.y = E::pack2(acc[2 * g][j][2], acc[2 * g][j][3]);
        pk.z = E::pack2(acc[2 * g + 1][j][0], acc[2 * g + 1][j][1]);
        pk.w = E::pack2(acc[2 * g + 1][j][2], acc[2 * g + 1][j][3]);
        // K % 8 == 0: a group of 8 channels is wholly in or out
        if (m < M && ch < K) *(uint4*)(y + (int64_t)m * K + ch) = pk;
      }
    }
  }
}

// chunk swizzle of a [pixel][64 ch] (128-byte row) LDS image read by ds_read_b64_tr_b16 (pwconv.hip's)
PDT_DEVICE int st_tr_swz(int row) { return (((row >> 1) & 1) << 1) | (((row >> 3) & 1) << 2); }

template <int DT>
__global__ __launch_bounds__(256) void stem3x3_wgrad_kernel(const float* __restrict__ x,
                                                            const uint16_t* __restrict__ dy, float* __restrict__ ws,
                                                            int M, int H, int W, int K, int P, int Q, FastDiv dQ,
                                                            FastDiv dP, int pps) {
  using E = E16<DT>;
  typedef typename E::vec8 vec8;
  constexpr int BKP = 128;        // pixels per reduction step
  constexpr int ROWB = 128;       // bytes of an LDS row: 64 values (the patch uses the first 32 of its rows)
  constexpr int XB = BKP * ROWB;  // bytes of one operand's tile
  constexpr int STAGE = 2 * XB;   // [patch | dy]
  __shared__ __attribute__((aligned(1024))) char smem[2 * STAGE];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int split = blockIdx.x;
  const int pix_begin = split * pps;
  const int pix_end = min(M, pix_begin + pps);
  const int nsteps = (pix_end - pix_begin + BKP - 1) / BKP;

  // dy staging (pwconv.hip's): piece (wave * 4 + j) is 8 rows x 8 chunks = 1 KiB, LDS chunk pch of a row holds the
  // source chunk pch ^ swz(row); a row past the split's range or a chunk past K loads zeros (kOOB)
  const int lrow = lane >> 3, pch = lane & 7;
  // patch staging: item e * 256 + tid is chunk tid & 3 of row (e * 256 + tid) >> 2
  const int xch = tid & 3;
  const StemTaps taps = stem_taps(xch, W);
  // two register sets: the loads of steps s + 1 and s + 2 are in flight while step s is multiplied
  uint4 ry[2][4];
  float xv[2][2][8];
  uint32_t xm[2][2];
  // a step past the split's range has no rows: every dy offset is kOOB against an empty resource and every image
  // index is 0 (zeros reach the registers, nothing outside the operands is touched)
  auto gload = [&](int step, int set) {
    const int pb = pix_begin + step * BKP;
    const int rows = max(0, min(BKP, pix_end - pb));
    const __amdgpu_buffer_rsrc_t rsy = make_rsrc(dy + (int64_t)pb * K, (uint32_t)(rows * K * 2));
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int row = (wave * 4 + j) * 8 + lrow;
      const int k = (pch ^ st_tr_swz(row)) * 8;
      ry[set][j] = st_load16(rsy, (row < rows && k < K) ? (uint32_t)((row * K + k) * 2) : kOOB);
    }
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const int row = (e * 256 + tid) >> 2;
      const bool live = row < rows;
      const StemPix px = stem_pixel(x, (uint32_t)(pb + row), live, H, W, P, Q, dQ, dP);
      xm[set][e] = stem_load8(px, live, H, W, taps, xv[set][e]);
    }
  };
  auto lstore = [&](int buf, int set) {
    char* sb = smem + buf * STAGE;
#pragma unroll
    for (int j = 0; j < 4; ++j) *(uint4*)(sb + XB + (wave * 4 + j) * 1024 + lane * 16) = ry[set][j];
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const int row = (e * 256 + tid) >> 2;
      *(uint4*)(sb + row * ROWB + ((xch ^ st_tr_swz(row)) << 4)) = stem_pack8<DT>(xv[set][e], xm[set][e]);
    }
  };

  f32x4_t acc[2][4];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  // transposed-read lane geometry: group g = lane >> 4 holds pixels 8g .. 8g + 7 of the wave's 32-pixel slice
  const int g = lane >> 4, li = lane & 15, q = li >> 2, p4 = li & 3;
  auto frag = [&](const char* base, int f) {
    const int r0 = wave * 32 + 8 * g + q, r1 = r0 + 4;
    const int col = f * 16 + 4 * p4;  // element within the 64-wide row
    const int ch = col >> 3, off = (col & 7) * 2;
    const int o0 = r0 * ROWB + ((ch ^ st_tr_swz(r0)) << 4) + off;
    const int o1 = r1 * ROWB + ((ch ^ st_tr_swz(r1)) << 4) + off;
    const s16x4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((st_lds_s16x4*)(base + o0));
    const s16x4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((st_lds_s16x4*)(base + o1));
    return __builtin_bit_cast(vec8, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
  };

  auto multiply = [&](int buf) {
    const char* sb = smem + buf * STAGE;
    vec8 af[2], bfr[4];
#pragma unroll
    for (int f = 0; f < 2; ++f) af[f] = frag(sb, f);
#pragma unroll
    for (int f = 0; f < 4; ++f)
      if (16 * f < K) bfr[f] = frag(sb + XB, f);  // wave-uniform: fragments past K are neither read nor used
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (16 * j < K) acc[i][j] = E::mfma16x16x32(af[i], bfr[j], acc[i][j]);
  };

  if (nsteps > 0) {  // block-uniform
    gload(0, 0);
    gload(1, 1);
    lstore(0, 0);
    __syncthreads();
    for (int s = 0; s < nsteps; s += 2) {
      // LDS buffer 0 holds step s, set 1 step s + 1 (in flight), set 0 is free
      gload(s + 2, 0);
      multiply(0);
      lstore(1, 1);  // the other buffer: last read before the previous barrier
      __syncthreads();
      if (s + 1 >= nsteps) break;
      // LDS buffer 1 holds step s + 1, set 0 step s + 2 (in flight), set 1 is free
      gload(s + 3, 1);
      multiply(1);
      lstore(0, 0);
      __syncthreads();
    }
  }

  // sum the 4 waves' tiles through LDS in wave order; acc[i][j]: rows c = 16i + 4 * (lane >> 4) + r (the reduction
  // slot j of the header: 27..31 are exact zeros), col k = 16j + (lane & 15)
  float* red = (float*)smem;  // [4 waves][64 k][32 c]
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int k = 16 * j + (lane & 15);
      const int c = 16 * i + 4 * (lane >> 4);
      *(f32x4_t*)(red + (wave * 64 + k) * 32 + c) = acc[i][j];
    }
  __syncthreads();
  float* slab = ws + (int64_t)split * K * kStemRedPad;
#pragma unroll
  for (int e = 0; e < 2; ++e) {
    const int idx = (e * 256 + tid) * 4;  // 0 .. 2047
    const int k = idx >> 5, c = idx & 31;
    f32x4_t v = *(f32x4_t*)(red + k * 32 + c);
#pragma unroll
    for (int wv = 1; wv < 4; ++wv) v += *(f32x4_t*)(red + (wv * 64 + k) * 32 + c);
    if (k < K) *(f32x4_t*)(slab + k * kStemRedPad + c) = v;
  }
}

// persistent blocks the forward aims for: a few per CU (256 CUs)
constexpr int kStemFwdBlocks = 2048;

template <int DT, int NG>
void stem_fwd_go(const float* x, const uint16_t* w, uint16_t* y, int64_t N, int H, int W, int K, hipStream_t s) {
  constexpr int PT = 4;
  const int P = (int)stem3x3_out(H), Q = (int)stem3x3_out(W);
  const int64_t M = N * P * Q, BR = 4 * PT * 16;
  const int mtiles = (int)((M + BR - 1) / BR);
  const dim3 g((unsigned)(mtiles < kStemFwdBlocks ? mtiles : kStemFwdBlocks));
  hipLaunchKernelGGL((stem3x3_fwd_kernel<DT, NG, PT>), g, dim3(256), 0, s, x, w, y, (int)M, H, W, K, P, Q,
                     make_fastdiv((uint32_t)Q), make_fastdiv((uint32_t)P), mtiles);
}

template <int DT>
void stem_wgrad_go(const float* x, const uint16_t* dy, float* ws, int64_t N, int H, int W, int K,
                   const StemWgradPlan& plan, hipStream_t s) {
  const int P = (int)stem3x3_out(H), Q = (int)stem3x3_out(W);
  hipLaunchKernelGGL((stem3x3_wgrad_kernel<DT>), dim3((unsigned)plan.splits), dim3(256), 0, s, x, dy, ws,
                     (int)(N * P * Q), H, W, K, P, Q, make_fastdiv((uint32_t)Q), make_fastdiv((uint32_t)P),
                     plan.pix_per_split);
}

}  // namespace

void stem3x3_fwd_launch(int dtype, const float* x, const uint16_t* w, uint16_t* y, int64_t N, int H, int W, int K,
                        hipStream_t s) {
  if (!stem3x3_fits(N, H, W, K)) pdt_hip_fail("stem3x3_fwd_launch: geometry outside the kernels' contract", hipErrorInvalidValue, __FILE__, __LINE__);
  PDT_COUNT("stem3x3_fwd");
  if (dtype == kBF16) {
    if (K <= 32) stem_fwd_go<kBF16, 1>(x, w, y, N, H, W, K, s);
    else stem_fwd_go<kBF16, 2>(x, w, y, N, H, W, K, s);
  } else {
    if (K <= 32) stem_fwd_go<kF16, 1>(x, w, y, N, H, W, K, s);
    else stem_fwd_go<kF16, 2>(x, w, y, N, H, W, K, s);
  }
}

StemWgradPlan stem3x3_wgrad_plan(int64_t M, int K, int target_blocks) {
  (void)K;  // one block owns the whole [K][32] tile of its split
  StemWgradPlan pl{};
  int64_t splits = target_blocks;
  const int64_t most = (M + 127) / 128;  // at least one reduction step per split
  if (splits > most) splits = most;
  if (splits > 4096) splits = 4096;  // bounds the slab workspace
  if (splits < 1) splits = 1;
  int64_t pps = M > 0 ? (M + splits - 1) / splits : 128;
  pps = (pps + 127) / 128 * 128;
  pl.pix_per_split = (int)pps;
  pl.splits = M > 0 ? (int)((M + pps - 1) / pps) : 1;
  return pl;
}

void stem3x3_wgrad_launch(int dtype, const float* x, const uint16_t* dy, float* ws, int64_t N, int H, int W, int K,
                          const StemWgradPlan& plan, hipStream_t s) {
  if (!stem3x3_fits(N, H, W, K)) pdt_hip_fail("stem3x3_wgrad_launch: geometry outside the kernels' contract", hipErrorInvalidValue, __FILE__, __LINE__);
  const int64_t M = N * stem3x3_out(H) * stem3x3_out(W);
  if (plan.splits < 1 || plan.pix_per_split < 128 || plan.pix_per_split % 128 != 0 ||
      (int64_t)plan.splits * plan.pix_per_split < M || (int64_t)(plan.splits - 1) * plan.pix_per_split >= M)
    pdt_hip_fail("stem3x3_wgrad_launch: the plan does not cover the pixels", hipErrorInvalidValue, __FILE__, __LINE__);
  PDT_COUNT("stem3x3_wgrad");
  if (dtype == kBF16) stem_wgrad_go<kBF16>(x, dy, ws, N, H, W, K, plan, s);
  else stem_wgrad_go<kF16>(x, dy, ws, N, H, W, K, plan, s);
}

}  // namespace pdt
