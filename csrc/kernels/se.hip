// Squeeze-and-excitation for the torch engine (SURVEY §2.2 model registry: EfficientNet / V2, MobileNetV3, RegNet-Y,
// MaxViT's MBConv): y = x * gate(W2 act(W1 mean_hw(x) + b1) + b2) over a dense NHWC x[N][HW][C], 16-bit, C % 8 == 0,
// 8 <= C <= 4096, 1 <= S <= 512.  The forward reads x twice and writes y once, the backward reads dy and x, then dy
// again, and writes dx once; everything between the passes lives in fp32 vectors per image.
//
// Work split:
//   * the two reductions (se_pool: sum x; se_bwd_reduce: sum dy * x) use the lane layout of col_reduce.h, per image: a
//     lane owns 8 consecutive channels (one 16-byte load per row), a 256-thread block is cvb channel groups x rpi row
//     lanes, blockIdx.x is a chunk of HW rows (SePlan), blockIdx.y the image, blockIdx.z a column chunk (only C > 2048
//     has two).  The row lanes are folded through LDS in lane order and the block writes one fp32 row of
//     partial[N][chunks][C]; the gate kernels fold the chunks in index order.  (col_reduce.h itself takes blockIdx.y
//     for the column chunk and writes one row per blockIdx.x: it does not fit unchanged.)
//   * se_gate / se_gate_bwd: one block per group of IMG images (4, or 2 when 4 do not fit in 64 KiB of LDS), so W1
//     and W2 are read once per block.  z (dv) sits in LDS.  W1 z: a wave per output, lanes stride over C with
//     coalesced reads of the row, xor-tree wave sum.  W2 h: a thread per channel loops over S.  W2^T dv: lanes are SB
//     consecutive s (coalesced rows of W2) x 256 / SB channel lanes, folded through LDS in lane order.  W1^T du: a
//     thread per channel, coalesced across the threads.
//   * se_scale / se_bwd_apply: persistent streaming blocks in the same lane layout; an item is kU * rpi rows of one
//     image, kU 16-byte vectors in flight per thread, the image's gate for the lane's 8 channels from L2; the block
//     steps through (image, tile) without a division in the loop.
//   * se_wgrad: one thread per element of dW2 | dW1 | db2 | db1, looping over the images in index order.
// sigmoid(v) = 1 / (1 + exp2(-v log2 e)) on the exp2 and reciprocal units (1 ulp each; exp2 flushes subnormals).
#include "../common.h"
#include "se.h"

namespace pdt {

namespace {

constexpr int kRU = 4;         // rows in flight per thread in the reductions
constexpr int kU = 4;          // vectors in flight per thread in the streaming passes
constexpr int kMinRows = 8;    // rows per thread a chunk should have before HW is split further
constexpr int kMinChunk = 64;  // ... and rows a chunk should have at all: a 7 x 7 map is one chunk at any width
constexpr int kMaxGridY = 65535;
constexpr float kLog2e = 1.4426950408889634f;

struct SeLanes {
  int cvb, rpi, zc;  // channel groups per block, row lanes per block, column chunks
};
SeLanes se_lanes(int C) {
  const int groups = C / 8, cvb = groups < 256 ? groups : 256;
  return SeLanes{cvb, 256 / cvb, (groups + cvb - 1) / cvb};
}

PDT_DEVICE float se_sigmoid(float v) { return __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(-v * kLog2e)); }

template <int ACT>
PDT_DEVICE float se_act(float u) {
  if constexpr (ACT == kSeRelu) return u > 0.f ? u : 0.f;
  return u * se_sigmoid(u);
}
template <int ACT>
PDT_DEVICE float se_act_grad(float u) {
  if constexpr (ACT == kSeRelu) return u > 0.f ? 1.f : 0.f;
  const float sg = se_sigmoid(u);
  return sg * (1.f + u * (1.f - sg));
}
template <int GATE>
PDT_DEVICE float se_gate(float v) {
  if constexpr (GATE == kSeSigmoid) return se_sigmoid(v);
  return fminf(fmaxf(fmaf(v, 1.f / 6.f, 0.5f), 0.f), 1.f);
}
// from the stored gate: sigmoid' = s (1 - s); hardsigmoid' = 1/6 inside (0, 1), torch's -3 < v < 3
template <int GATE>
PDT_DEVICE float se_gate_grad(float sg) {
  if constexpr (GATE == kSeSigmoid) return sg * (1.f - sg);
  return (sg > 0.f && sg < 1.f) ? 1.f / 6.f : 0.f;
}

PDT_DEVICE void load8f(const float* p, float (&o)[8]) {
  const float4 a = *(const float4*)p, b = *(const float4*)(p + 4);
  o[0] = a.x; o[1] = a.y; o[2] = a.z; o[3] = a.w;
  o[4] = b.x; o[5] = b.y; o[6] = b.z; o[7] = b.w;
}

// ------------------------------------------------------------------------------- se_pool / se_bwd_reduce
// OPS = 1: sums of a; OPS = 2: sums of a * b.  grid (chunks, min(N, 65535), zc)
template <int DT, int OPS, bool NT>
__global__ __launch_bounds__(256) void se_reduce_kernel(const uint16_t* __restrict__ a, const uint16_t* __restrict__ b,
                                                        float* __restrict__ partial, int64_t N, int64_t HW, int C,
                                                        int cvb, int rpi, int64_t rpc) {
  using E = E16<DT>;
  __shared__ float red[256 * 8];
  const int cl = threadIdx.x % cvb, rl = threadIdx.x / cvb;
  const int per = cvb * 8, col0 = blockIdx.z * per;
  const int c0 = col0 + cl * 8;
  const bool active = rl < rpi && c0 < C;
  const int64_t r0 = (int64_t)blockIdx.x * rpc, r1 = r0 + rpc < HW ? r0 + rpc : HW;
  const int64_t step = rpi;
  for (int64_t n = blockIdx.y; n < N; n += gridDim.y) {
    if (active) {
      float s[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) s[e] = 0.f;
      const int64_t base = n * HW * C + c0;
      for (int64_t r = r0 + rl; r < r1; r += step * kRU) {
        uint4 av[kRU], bv[kRU];
#pragma unroll
        for (int j = 0; j < kRU; ++j)
          if (r + j * step < r1) {
            av[j] = ld16<NT>(a + base + (r + j * step) * C);
            if constexpr (OPS == 2) bv[j] = ld16<NT>(b + base + (r + j * step) * C);
          }
#pragma unroll
        for (int j = 0; j < kRU; ++j) {
          if (r + j * step >= r1) break;
          uint16_t ah[8], bh[8];
          unpack8(av[j], ah);
          if constexpr (OPS == 2) unpack8(bv[j], bh);
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            if constexpr (OPS == 2) s[e] = fmaf(E::to_f(ah[e]), E::to_f(bh[e]), s[e]);
            else s[e] += E::to_f(ah[e]);
          }
        }
      }
#pragma unroll
      for (int e = 0; e < 8; ++e) red[(rl * cvb + cl) * 8 + e] = s[e];
    }
    __syncthreads();
    float* dst = partial + (n * gridDim.x + blockIdx.x) * C + col0;
    for (int idx = threadIdx.x; idx < per && col0 + idx < C; idx += 256) {
      float t = 0.f;
      for (int r = 0; r < rpi; ++r) t += red[r * per + idx];
      dst[idx] = t;
    }
    __syncthreads();
  }
}

// ------------------------------------------------------------------------------------------------ se_gate
// dynamic LDS: zs[IMG][C] | hs[IMG][S]
template <int ACT, int GATE, int IMG>
__global__ __launch_bounds__(256) void se_gate_kernel(const float* __restrict__ partial, const float* __restrict__ w1,
                                                      const float* __restrict__ b1, const float* __restrict__ w2,
                                                      const float* __restrict__ b2, float* __restrict__ z,
                                                      float* __restrict__ u, float* __restrict__ sg, int64_t N, int C,
                                                      int S, int chunks, float inv_hw) {
  extern __shared__ float se_lds[];
  float* zs = se_lds;
  float* hs = se_lds + IMG * C;
  const int64_t n0 = (int64_t)blockIdx.x * IMG;
  for (int idx = threadIdx.x; idx < IMG * C; idx += 256) {
    const int i = idx / C, c = idx - i * C;
    const int64_t n = n0 + i;
    float v = 0.f;
    if (n < N) {
      const float* p = partial + n * chunks * C + c;
      float t = 0.f;
      for (int k = 0; k < chunks; ++k) t += p[(int64_t)k * C];
      v = t * inv_hw;
      z[n * C + c] = v;
    }
    zs[idx] = v;
  }
  __syncthreads();
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int so = wave; so < S; so += 4) {  // uniform per wave: every lane shuffles
    float acc[IMG];
#pragma unroll
    for (int i = 0; i < IMG; ++i) acc[i] = 0.f;
    const float* wr = w1 + (int64_t)so * C;
#pragma unroll 4
    for (int c = lane; c < C; c += 64) {
      const float w = wr[c];
#pragma unroll
      for (int i = 0; i < IMG; ++i) acc[i] = fmaf(w, zs[i * C + c], acc[i]);
    }
    const float bias = b1[so];
#pragma unroll
    for (int i = 0; i < IMG; ++i) {
      const float t = wave_sum(acc[i]) + bias;
      if (lane == 0) {
        if (n0 + i < N) u[(n0 + i) * S + so] = t;
        hs[i * S + so] = se_act<ACT>(t);
      }
    }
  }
  __syncthreads();
  for (int c = threadIdx.x; c < C; c += 256) {
    float acc[IMG];
#pragma unroll
    for (int i = 0; i < IMG; ++i) acc[i] = 0.f;
    const float* wr = w2 + (int64_t)c * S;
#pragma unroll 4
    for (int so = 0; so < S; ++so) {
      const float w = wr[so];
#pragma unroll
      for (int i = 0; i < IMG; ++i) acc[i] = fmaf(w, hs[i * S + so], acc[i]);
    }
    const float bias = b2[c];
#pragma unroll
    for (int i = 0; i < IMG; ++i)
      if (n0 + i < N) sg[(n0 + i) * C + c] = se_gate<GATE>(acc[i] + bias);
  }
}

// -------------------------------------------------------------------------------------------- se_gate_bwd
// dynamic LDS: dvs[IMG][C] | dus[IMG][S] | red[IMG][256 / SB][SB]; SB = 1 << sbshift consecutive s per channel lane
template <int ACT, int GATE, int IMG>
__global__ __launch_bounds__(256) void se_gate_bwd_kernel(const float* __restrict__ partial,
                                                          const float* __restrict__ w1, const float* __restrict__ w2,
                                                          const float* __restrict__ u, const float* __restrict__ sg,
                                                          float* __restrict__ dv, float* __restrict__ du,
                                                          float* __restrict__ g, int64_t N, int C, int S, int chunks,
                                                          float inv_hw, int sbshift) {
  extern __shared__ float se_lds[];
  float* dvs = se_lds;
  float* dus = se_lds + IMG * C;
  float* red = dus + IMG * S;
  const int64_t n0 = (int64_t)blockIdx.x * IMG;
  for (int idx = threadIdx.x; idx < IMG * C; idx += 256) {
    const int i = idx / C, c = idx - i * C;
    const int64_t n = n0 + i;
    float d = 0.f;
    if (n < N) {
      const float* p = partial + n * chunks * C + c;
      float t = 0.f;
      for (int k = 0; k < chunks; ++k) t += p[(int64_t)k * C];
      d = t * se_gate_grad<GATE>(sg[n * C + c]);
      dv[n * C + c] = d;
    }
    dvs[idx] = d;
  }
  __syncthreads();
  const int SB = 1 << sbshift, ncl = 256 >> sbshift;
  const int sl = threadIdx.x & (SB - 1), cl = threadIdx.x >> sbshift;
  for (int s0 = 0; s0 < S; s0 += SB) {  // uniform per block
    float acc[IMG];
#pragma unroll
    for (int i = 0; i < IMG; ++i) acc[i] = 0.f;
    if (s0 + sl < S) {
      const float* wc = w2 + s0 + sl;
#pragma unroll 4
      for (int c = cl; c < C; c += ncl) {
        const float w = wc[(int64_t)c * S];
#pragma unroll
        for (int i = 0; i < IMG; ++i) acc[i] = fmaf(w, dvs[i * C + c], acc[i]);
      }
    }
#pragma unroll
    for (int i = 0; i < IMG; ++i) red[(i * ncl + cl) * SB + sl] = acc[i];
    __syncthreads();
    if ((int)threadIdx.x < IMG * SB) {
      const int i = threadIdx.x >> sbshift, so = s0 + sl;
      if (so < S) {
        float t = 0.f;
        for (int r = 0; r < ncl; ++r) t += red[(i * ncl + r) * SB + sl];
        float d = 0.f;
        if (n0 + i < N) {
          d = t * se_act_grad<ACT>(u[(n0 + i) * S + so]);
          du[(n0 + i) * S + so] = d;
        }
        dus[i * S + so] = d;
      }
    }
    __syncthreads();
  }
  for (int c = threadIdx.x; c < C; c += 256) {
    float acc[IMG];
#pragma unroll
    for (int i = 0; i < IMG; ++i) acc[i] = 0.f;
#pragma unroll 4
    for (int so = 0; so < S; ++so) {
      const float w = w1[(int64_t)so * C + c];
#pragma unroll
      for (int i = 0; i < IMG; ++i) acc[i] = fmaf(w, dus[i * S + so], acc[i]);
    }
#pragma unroll
    for (int i = 0; i < IMG; ++i)
      if (n0 + i < N) g[(n0 + i) * C + c] = acc[i] * inv_hw;
  }
}

// ------------------------------------------------------------------------------------------------ se_wgrad
// element idx of dW2[C][S] | dW1[S][C] | db2[C] | db1[S]
template <int ACT>
__global__ __launch_bounds__(256) void se_wgrad_kernel(const float* __restrict__ dv, const float* __restrict__ du,
                                                       const float* __restrict__ z, const float* __restrict__ u,
                                                       float* __restrict__ dw1, float* __restrict__ db1,
                                                       float* __restrict__ dw2, float* __restrict__ db2, int64_t N,
                                                       int C, int S) {
  const int CS = C * S;
  const int idx = blockIdx.x * 256 + threadIdx.x;
  float t = 0.f;
  if (idx < CS) {
    const int c = idx / S, so = idx - c * S;
    for (int64_t n = 0; n < N; ++n) t = fmaf(dv[n * C + c], se_act<ACT>(u[n * S + so]), t);
    dw2[idx] = t;
  } else if (idx < 2 * CS) {
    const int j = idx - CS, so = j / C, c = j - so * C;
    for (int64_t n = 0; n < N; ++n) t = fmaf(du[n * S + so], z[n * C + c], t);
    dw1[j] = t;
  } else if (idx < 2 * CS + C) {
    const int c = idx - 2 * CS;
    for (int64_t n = 0; n < N; ++n) t += dv[n * C + c];
    db2[c] = t;
  } else if (idx < 2 * CS + C + S) {
    const int so = idx - 2 * CS - C;
    for (int64_t n = 0; n < N; ++n) t += du[n * S + so];
    db1[so] = t;
  }
}

// ------------------------------------------------------------------------------- se_scale / se_bwd_apply
// out = round(a * sg) (BWD: round(a * sg + g)).  grid (persistent blocks, zc); item = tile `t` of kU * rpi rows of
// image `n`, items = N * tpi
template <int DT, bool BWD, bool NT>
__global__ __launch_bounds__(256) void se_apply_kernel(const uint16_t* __restrict__ a, const float* __restrict__ sg,
                                                       const float* __restrict__ g, uint16_t* __restrict__ out,
                                                       int64_t HW, int C, int cvb, int rpi, int64_t tpi,
                                                       int64_t items) {
  using E = E16<DT>;
  const int cl = threadIdx.x % cvb, rl = threadIdx.x / cvb;
  const int c0 = (blockIdx.y * cvb + cl) * 8;
  if (!(rl < rpi && c0 < C)) return;
  int64_t n = blockIdx.x / tpi, t = blockIdx.x - n * tpi;
  const int64_t sn = gridDim.x / tpi, st = gridDim.x - sn * tpi;
  for (int64_t it = blockIdx.x; it < items; it += gridDim.x) {
    const int64_t r0 = t * (kU * rpi) + rl;
    const int64_t base = n * HW * C + c0;
    uint4 v[kU];
#pragma unroll
    for (int k = 0; k < kU; ++k)
      if (r0 + k * rpi < HW) v[k] = ld16<NT>(a + base + (r0 + k * rpi) * C);
    float sc[8], sh[8];
    load8f(sg + n * C + c0, sc);
    if constexpr (BWD) load8f(g + n * C + c0, sh);
#pragma unroll
    for (int k = 0; k < kU; ++k) {
      const int64_t r = r0 + k * rpi;
      if (r >= HW) break;
      uint16_t h[8];
      unpack8(v[k], h);
      float o[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        if constexpr (BWD) o[e] = fmaf(E::to_f(h[e]), sc[e], sh[e]);
        else o[e] = E::to_f(h[e]) * sc[e];
      }
      st16<NT>(out + base + r * C,
               make_uint4(E::pack2(o[0], o[1]), E::pack2(o[2], o[3]), E::pack2(o[4], o[5]), E::pack2(o[6], o[7])));
    }
    t += st;
    n += sn;
    if (t >= tpi) {
      t -= tpi;
      ++n;
    }
  }
}

void check_shape(const char* what, int dtype, int64_t N, int64_t HW, int C, int S) {
  if ((dtype != kBF16 && dtype != kF16) || !se_fits(N, HW, C, S)) pdt_hip_fail(what, hipErrorInvalidValue, __FILE__, __LINE__);
}

// images per gate block and the kernel's dynamic LDS bytes (`extra` floats per image group beside [IMG][C + S])
int gate_images(int C, int S, int extra) { return (size_t)(4 * (C + S) + extra) * sizeof(float) <= 65536 ? 4 : 2; }

template <int DT, int OPS>
void reduce_launch(const uint16_t* a, const uint16_t* b, float* partial, int64_t N, int64_t HW, int C, const SePlan& p,
                   hipStream_t s) {
  const SeLanes ln = se_lanes(C);
  if (p.chunks < 1 || p.rows_per_chunk < 1 || p.chunks * p.rows_per_chunk < HW || (p.chunks - 1) * p.rows_per_chunk >= HW)
    pdt_hip_fail("se reduce: the plan does not cover HW", hipErrorInvalidValue, __FILE__, __LINE__);
  const dim3 grid((unsigned)p.chunks, (unsigned)(N < kMaxGridY ? N : kMaxGridY), (unsigned)ln.zc);
  if (ew_nt(N * HW * C * 2))
    hipLaunchKernelGGL((se_reduce_kernel<DT, OPS, true>), grid, dim3(256), 0, s, a, b, partial, N, HW, C, ln.cvb, ln.rpi,
                       p.rows_per_chunk);
  else
    hipLaunchKernelGGL((se_reduce_kernel<DT, OPS, false>), grid, dim3(256), 0, s, a, b, partial, N, HW, C, ln.cvb,
                       ln.rpi, p.rows_per_chunk);
}

template <int DT, bool BWD>
void apply_launch(const uint16_t* a, const float* sg, const float* g, uint16_t* out, int64_t N, int64_t HW, int C,
                  int max_blocks, hipStream_t s) {
  const SeLanes ln = se_lanes(C);
  const int64_t tile = (int64_t)kU * ln.rpi, tpi = (HW + tile - 1) / tile, items = N * tpi;
  const int64_t cap = max_blocks < 1 ? 1 : max_blocks;
  const dim3 grid((unsigned)(items < cap ? items : cap), (unsigned)ln.zc);
  if (ew_nt(N * HW * C * 2))
    hipLaunchKernelGGL((se_apply_kernel<DT, BWD, true>), grid, dim3(256), 0, s, a, sg, g, out, HW, C, ln.cvb, ln.rpi,
                       tpi, items);
  else
    hipLaunchKernelGGL((se_apply_kernel<DT, BWD, false>), grid, dim3(256), 0, s, a, sg, g, out, HW, C, ln.cvb, ln.rpi,
                       tpi, items);
}

}  // namespace

bool se_fits(int64_t N, int64_t HW, int64_t C, int64_t S) {
  if (N < 1 || HW < 1 || C < 8 || C > 4096 || C % 8 != 0 || S < 1 || S > 512) return false;
  if (HW >= (int64_t(1) << 40) || N >= (int64_t(1) << 40)) return false;  // the products below cannot overflow
  return HW * C < (int64_t(1) << 40) && N <= ((int64_t(1) << 40) - 1) / (HW * C);
}

SePlan se_plan(int64_t N, int64_t HW, int C, int max_blocks) {
  const SeLanes ln = se_lanes(C);
  const int64_t cap = max_blocks < 1 ? 1 : max_blocks;
  int64_t per_img = cap / (N * ln.zc);  // what the cap leaves an image
  if (per_img < 1) per_img = 1;
  int64_t min_rows = (int64_t)ln.rpi * kMinRows;
  if (min_rows < kMinChunk) min_rows = kMinChunk;
  int64_t chunks = (HW + min_rows - 1) / min_rows;
  if (chunks > per_img) chunks = per_img;
  const int64_t rpc = (HW + chunks - 1) / chunks;
  return SePlan{(int)((HW + rpc - 1) / rpc), rpc};  // no empty chunk
}

void se_pool_launch(int dtype, const uint16_t* x, float* partial, int64_t N, int64_t HW, int C, const SePlan& plan,
                    hipStream_t s) {
  check_shape("se_pool_launch: arguments outside the kernels' contract", dtype, N, HW, C, 1);
  PDT_COUNT("se_pool");
  if (dtype == kBF16) reduce_launch<kBF16, 1>(x, nullptr, partial, N, HW, C, plan, s);
  else reduce_launch<kF16, 1>(x, nullptr, partial, N, HW, C, plan, s);
}

void se_bwd_reduce_launch(int dtype, const uint16_t* dy, const uint16_t* x, float* partial, int64_t N, int64_t HW, int C,
                          const SePlan& plan, hipStream_t s) {
  check_shape("se_bwd_reduce_launch: arguments outside the kernels' contract", dtype, N, HW, C, 1);
  PDT_COUNT("se_bwd_reduce");
  if (dtype == kBF16) reduce_launch<kBF16, 2>(dy, x, partial, N, HW, C, plan, s);
  else reduce_launch<kF16, 2>(dy, x, partial, N, HW, C, plan, s);
}

void se_scale_launch(int dtype, const uint16_t* x, const float* sg, uint16_t* y, int64_t N, int64_t HW, int C,
                     int max_blocks, hipStream_t s) {
  check_shape("se_scale_launch: arguments outside the kernels' contract", dtype, N, HW, C, 1);
  PDT_COUNT("se_scale");
  if (dtype == kBF16) apply_launch<kBF16, false>(x, sg, nullptr, y, N, HW, C, max_blocks, s);
  else apply_launch<kF16, false>(x, sg, nullptr, y, N, HW, C, max_blocks, s);
}

void se_bwd_apply_launch(int dtype, const uint16_t* dy, const float* sg, const float* g, uint16_t* dx, int64_t N,
                         int64_t HW, int C, int max_blocks, hipStream_t s) {
  check_shape("se_bwd_apply_launch: arguments outside the kernels' contract", dtype, N, HW, C, 1);
  PDT_COUNT("se_bwd_apply");
  if (dtype == kBF16) apply_launch<kBF16, true>(dy, sg, g, dx, N, HW, C, max_blocks, s);
  else apply_launch<kF16, true>(dy, sg, g, dx, N, HW, C, max_blocks, s);
}

// dispatch KERNEL<ACT, GATE, IMG> over the runtime (act, gate, img); falls through when nothing matches
#define PDT_SE_CASE(KERNEL, ACT_, GATE_, IMG_, ...)                                                              \
  if (act == ACT_ && gate == GATE_ && img == IMG_) {                                                             \
    hipLaunchKernelGGL((KERNEL<ACT_, GATE_, IMG_>), grid, dim3(256), lds, s, __VA_ARGS__);                       \
    launched_ = true;                                                                                            \
  }
#define PDT_SE_DISPATCH(KERNEL, ...)                                                                             \
  bool launched_ = false;                                                                                        \
  PDT_SE_CASE(KERNEL, kSeRelu, kSeSigmoid, 4, __VA_ARGS__) PDT_SE_CASE(KERNEL, kSeRelu, kSeSigmoid, 2, __VA_ARGS__) \
  PDT_SE_CASE(KERNEL, kSeRelu, kSeHardsigmoid, 4, __VA_ARGS__)                                                   \
  PDT_SE_CASE(KERNEL, kSeRelu, kSeHardsigmoid, 2, __VA_ARGS__)                                                   \
  PDT_SE_CASE(KERNEL, kSeSilu, kSeSigmoid, 4, __VA_ARGS__) PDT_SE_CASE(KERNEL, kSeSilu, kSeSigmoid, 2, __VA_ARGS__) \
  PDT_SE_CASE(KERNEL, kSeSilu, kSeHardsigmoid, 4, __VA_ARGS__)                                                   \
  PDT_SE_CASE(KERNEL, kSeSilu, kSeHardsigmoid, 2, __VA_ARGS__)

void se_gate_launch(int act, int gate, const float* partial, const float* w1, const float* b1, const float* w2,
                    const float* b2, float* z, float* u, float* sg, int64_t N, int64_t HW, int C, int S, int chunks,
                    hipStream_t s) {
  check_shape("se_gate_launch: arguments outside the kernels' contract", kBF16, N, HW, C, S);
  if (chunks < 1) pdt_hip_fail("se_gate_launch: chunks < 1", hipErrorInvalidValue, __FILE__, __LINE__);
  PDT_COUNT("se_gate");
  const int img = gate_images(C, S, 0);
  const size_t lds = (size_t)img * (C + S) * sizeof(float);
  const dim3 grid((unsigned)((N + img - 1) / img));
  const float inv_hw = 1.f / (float)HW;
  PDT_SE_DISPATCH(se_gate_kernel, partial, w1, b1, w2, b2, z, u, sg, N, C, S, chunks, inv_hw)
  if (!launched_) pdt_hip_fail("se_gate_launch: unsupported variant", hipErrorInvalidValue, __FILE__, __LINE__);
}

void se_gate_bwd_launch(int act, int gate, const float* partial, const float* w1, const float* w2, const float* u,
                        const float* sg, float* dv, float* du, float* g, int64_t N, int64_t HW, int C, int S, int chunks,
                        hipStream_t s) {
  check_shape("se_gate_bwd_launch: arguments outside the kernels' contract", kBF16, N, HW, C, S);
  if (chunks < 1) pdt_hip_fail("se_gate_bwd_launch: chunks < 1", hipErrorInvalidValue, __FILE__, __LINE__);
  PDT_COUNT("se_gate_bwd");
  const int img = gate_images(C, S, 4 * 256);
  const size_t lds = (size_t)(img * (C + S) + img * 256) * sizeof(float);
  const dim3 grid((unsigned)((N + img - 1) / img));
  const float inv_hw = 1.f / (float)HW;
  int sbshift = 0;
  while ((1 << sbshift) < S && sbshift < 6) ++sbshift;  // SB = the power of two >= min(S, 64)
  PDT_SE_DISPATCH(se_gate_bwd_kernel, partial, w1, w2, u, sg, dv, du, g, N, C, S, chunks, inv_hw, sbshift)
  if (!launched_) pdt_hip_fail("se_gate_bwd_launch: unsupported variant", hipErrorInvalidValue, __FILE__, __LINE__);
}
#undef PDT_SE_DISPATCH
#undef PDT_SE_CASE

void se_wgrad_launch(int act, const float* dv, const float* du, const float* z, const float* u, float* dw1, float* db1,
                     float* dw2, float* db2, int64_t N, int C, int S, hipStream_t s) {
  check_shape("se_wgrad_launch: arguments outside the kernels' contract", kBF16, N, 1, C, S);
  PDT_COUNT("se_wgrad");
  const dim3 grid((unsigned)((2 * C * S + C + S + 255) / 256));
  if (act == kSeRelu)
    hipLaunchKernelGGL((se_wgrad_kernel<kSeRelu>), grid, dim3(256), 0, s, dv, du, z, u, dw1, db1, dw2, db2, N, C, S);
  else if (act == kSeSilu)
    hipLaunchKernelGGL((se_wgrad_kernel<kSeSilu>), grid, dim3(256), 0, s, dv, du, z, u, dw1, db1, dw2, db2, N, C, S);
  else
    pdt_hip_fail("se_wgrad_launch: unsupported variant", hipErrorInvalidValue, __FILE__, __LINE__);
}

}  // namespace pdt
