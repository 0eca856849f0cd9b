// Window attention for the torch engine (SURVEY §2.2 model registry: every Swin, Swin V2 and MaxViT block):
//   y = softmax(scale * q k^T + bias [+ -100 where the region labels of query and key differ]) v
// over Bw windows of N <= 64 tokens, `heads` heads of dimension 32, 16-bit operands, fp32 math.  S and P never leave
// the wave: no K loop, no online softmax.
//
// Work split: one wave owns one (window, head) at a time; a block is 4 waves; blocks are persistent.  Wave
// gw = block * 4 + wave keeps head gw % heads (its 64 bias values per lane stay in registers) and walks the windows
// slot, slot + slabs, ... with slot = gw / heads.  Lane l = 16 g + c.
//   * S is computed transposed, 16 tiles of v_mfma_f32_16x16x32 with the head dimension as the one K step:
//     A = K (lane: key 16 jt + c, channels 8 g ..), B = Q^T (lane: query 16 it + c, channels 8 g ..) -- both are the
//     16-byte global loads as they come.  The four accumulators of tile (jt, it) are the keys 16 jt + 4 g + r of
//     query 16 it + c: a query's 64 keys sit in 4 lanes, so row max / row sum are an in-lane pass and two xor steps,
//     and the rounded P is the B operand (k = 4 g + r, n = c) of v_mfma_f32_16x16x16 as it stands.
//   * y^T = V^T P^T: A = V^T (lane: channel 16 dt + c, keys 16 jt + 4 g ..).  V is the one operand that has to be
//     transposed: each wave stages it through its own LDS tile [32][72] (2-byte writes, 8-byte reads).  The result
//     tile holds 4 consecutive channels of one query per lane: 8-byte stores into token-major y.
//   * backward: S^T and dP^T = V dO^T from the row loads the same way (16x16x32), P recomputed from the saved row
//     max / sum, D = sum_j P dP (in-lane + two xor steps), dS = P (dP - D) in fp32, added to the wave's dbias
//     registers unrounded.  dQ^T = K^T dS^T contracts over keys: dS from registers, K^T from the LDS tile.  dV^T =
//     dO^T P and dK^T = Q^T dS contract over queries, which lie across lanes: the rounded P, then the rounded dS, go
//     through a second per-wave LDS tile [64 keys][72] (2-byte writes) and come back as 16-byte B operands of the
//     16x16x32 MFMA, with dO^T / Q^T from the transposed tile as A.  All outputs: 4 channels of one token per lane.
//   * dbias: every wave writes its sums to partial[slot][head][N][N] (each (slot, head) is exactly one wave);
//     wgrad_reduce folds the slots in a fixed order.  No atomics.
// Keys >= N get -inf before the row max (p = 0 exactly).  Rows >= N are loaded as zeros and never stored: in the
// forward they carry a harmless uniform p, in the backward they get p = 0 so they add nothing to dV, dK or dbias.
#include <math.h>

#include "../common.h"
#include "winattn.h"

namespace pdt {

namespace {

constexpr int kLd = 72;  // 16-bit elements per LDS row: 64 tokens + 8 (144 bytes: 8- and 16-byte reads stay aligned)
constexpr float kLog2e = 1.4426950408889634f;

typedef _Float16 f16x4_t __attribute__((ext_vector_type(4)));

// v_mfma_f32_16x16x16: A[m = c][k = 4 g + r], B[k = 4 g + r][n = c], D[m = 4 g + r][n = c]
template <int DT>
PDT_DEVICE f32x4_t mma16(uint2 a, uint2 b, f32x4_t acc) {
  if constexpr (DT == kBF16)
    return __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(__builtin_bit_cast(s16x4_t, a), __builtin_bit_cast(s16x4_t, b),
                                                     acc, 0, 0, 0);
  else
    return __builtin_amdgcn_mfma_f32_16x16x16f16(__builtin_bit_cast(f16x4_t, a), __builtin_bit_cast(f16x4_t, b), acc,
                                                 0, 0, 0);
}

// v_mfma_f32_16x16x32: A[m = c][k = 8 g + e], B[k = 8 g + e][n = c], D[m = 4 g + r][n = c]
template <int DT>
PDT_DEVICE f32x4_t mma32(uint4 a, uint4 b, f32x4_t acc) {
  using V = typename E16<DT>::vec8;
  return E16<DT>::mfma16x16x32(__builtin_bit_cast(V, a), __builtin_bit_cast(V, b), acc);
}

template <int DT>
PDT_DEVICE uint2 pack4(float a, float b, float c, float d) {
  return make_uint2(E16<DT>::pack2(a, b), E16<DT>::pack2(c, d));
}

// Orders a wave's LDS writes before its own later LDS reads (and the reverse).  Every tile is private to one wave, and
// the LDS serves one wave's instructions in issue order, so no barrier between waves is needed: the fence only keeps
// the compiler from moving accesses of different lanes across it.
PDT_DEVICE void wa_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
}

struct WaLane {
  int c, g, h, slot;
};

// channels 8 g .. 8 g + 7 of token `tok` (zeros when !ok)
PDT_DEVICE uint4 wa_row(const WaOperand& o, int64_t w, const WaLane& t, int tok, bool ok) {
  if (!ok) return make_uint4(0u, 0u, 0u, 0u);
  return *(const uint4*)(o.p + w * o.sw + (int64_t)tok * o.st + (int64_t)t.h * o.sh + t.g * 8);
}

// the four row tiles of an operand into the transposed LDS tile T[channel][token]
PDT_DEVICE void wa_put_t(uint16_t* T, const uint4 (&rows)[4], const WaLane& t) {
#pragma unroll
  for (int tt = 0; tt < 4; ++tt) {
    uint16_t e[8];
    unpack8(rows[tt], e);
#pragma unroll
    for (int i = 0; i < 8; ++i) T[(t.g * 8 + i) * kLd + tt * 16 + t.c] = e[i];
  }
}

// 4 channels 16 dt + 4 g .. of token `tok`, scaled and rounded once
template <int DT>
PDT_DEVICE void wa_store4(const WaOperand& o, int64_t w, const WaLane& t, int tok, int dt, f32x4_t v, float scale) {
  *(uint2*)(o.p + w * o.sw + (int64_t)tok * o.st + (int64_t)t.h * o.sh + dt * 16 + t.g * 4) =
      pack4<DT>(v[0] * scale, v[1] * scale, v[2] * scale, v[3] * scale);
}

PDT_DEVICE WaLane wa_lane(int heads) {
  const int lane = threadIdx.x & 63, gw = (int)blockIdx.x * 4 + ((int)threadIdx.x >> 6);
  return WaLane{lane & 15, lane >> 4, gw % heads, gw / heads};
}

// the lane's bias values: [it][jt][r] = bias[h][16 it + c][16 jt + 4 g + r], zero outside N x N
PDT_DEVICE void wa_bias(const float* bias, const WaLane& t, int N, float (&b)[4][4][4]) {
#pragma unroll
  for (int it = 0; it < 4; ++it)
#pragma unroll
    for (int jt = 0; jt < 4; ++jt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = it * 16 + t.c, j = jt * 16 + t.g * 4 + r;
        b[it][jt][r] = (i < N && j < N) ? bias[((int64_t)t.h * N + i) * N + j] : 0.f;
      }
}

// region labels of the lane's 4 queries and 16 keys (0 where there is no region or past N)
PDT_DEVICE void wa_labels(const uint8_t* region, int nwin, int64_t w, const WaLane& t, int N, bool act, int (&lq)[4],
                          int (&lk)[4][4]) {
  const bool on = act && region != nullptr;
  const uint8_t* row = region + (on ? (w % nwin) * N : 0);
#pragma unroll
  for (int it = 0; it < 4; ++it) {
    const int i = it * 16 + t.c;
    lq[it] = (on && i < N) ? row[i] : 0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int j = it * 16 + t.g * 4 + r;
      lk[it][r] = (on && j < N) ? row[j] : 0;
    }
  }
}

// the 16 scores of query 16 it + c from its four S^T tiles: scale * s + bias (+ -100), -inf for keys >= N
PDT_DEVICE void wa_scores(const f32x4_t (&s)[4], const float (&b)[4][4], int lqi, const int (&lk)[4][4],
                          const WaLane& t, int N, float scale, float (&x)[4][4]) {
#pragma unroll
  for (int jt = 0; jt < 4; ++jt)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float v = s[jt][r] * scale + b[jt][r];
      if (lqi != lk[jt][r]) v += -100.f;
      x[jt][r] = (jt * 16 + t.g * 4 + r < N) ? v : -INFINITY;
    }
}

// over the 4 lanes (c, g = 0..3) that share a query
PDT_DEVICE float wa_qmax(float v) {
  v = fmaxf(v, __shfl_xor(v, 16, 64));
  return fmaxf(v, __shfl_xor(v, 32, 64));
}
PDT_DEVICE float wa_qsum(float v) {
  v += __shfl_xor(v, 16, 64);
  return v + __shfl_xor(v, 32, 64);
}

template <int DT>
__global__ __launch_bounds__(256) void winattn_fwd_kernel(const WaArgs a, int slabs, int iters) {
  __shared__ __attribute__((aligned(16))) uint16_t lds[4][32 * kLd];
  const WaLane t = wa_lane(a.heads);
  const int N = a.N;
  uint16_t* VT = lds[threadIdx.x >> 6];
  float bias[4][4][4];
  wa_bias(a.bias, t, N, bias);

  for (int it0 = 0; it0 < iters; ++it0) {
    const int64_t w = t.slot + (int64_t)it0 * slabs;
    const bool act = w < a.Bw;
    uint4 qr[4], kr[4], vr[4];
#pragma unroll
    for (int tt = 0; tt < 4; ++tt) {
      const int tok = tt * 16 + t.c;
      const bool ok = act && tok < N;
      qr[tt] = wa_row(a.q, w, t, tok, ok);
      kr[tt] = wa_row(a.k, w, t, tok, ok);
      vr[tt] = wa_row(a.v, w, t, tok, ok);
    }
    int lq[4], lk[4][4];
    wa_labels(a.region, a.nwin, w, t, N, act, lq, lk);
    wa_put_t(VT, vr, t);
    wa_lds_sync();
    uint2 vt[2][4];
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
      for (int jt = 0; jt < 4; ++jt) vt[dt][jt] = *(const uint2*)(VT + (dt * 16 + t.c) * kLd + jt * 16 + t.g * 4);

#pragma unroll
    for (int it = 0; it < 4; ++it) {
      const int i = it * 16 + t.c;
      f32x4_t s[4];
#pragma unroll
      for (int jt = 0; jt < 4; ++jt) s[jt] = mma32<DT>(kr[jt], qr[it], f32x4_t{0.f, 0.f, 0.f, 0.f});
      float x[4][4];
      wa_scores(s, bias[it], lq[it], lk, t, N, a.scale, x);
      float m = -INFINITY;
#pragma unroll
      for (int jt = 0; jt < 4; ++jt)
#pragma unroll
        for (int r = 0; r < 4; ++r) m = fmaxf(m, x[jt][r]);
      m = wa_qmax(m);  // key 0 is always real: m is finite
      float l = 0.f;
#pragma unroll
      for (int jt = 0; jt < 4; ++jt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          x[jt][r] = __builtin_amdgcn_exp2f((x[jt][r] - m) * kLog2e);
          l += x[jt][r];
        }
      l = wa_qsum(l);
      const float inv = 1.f / l;
      uint2 p[4];
#pragma unroll
      for (int jt = 0; jt < 4; ++jt)
        p[jt] = pack4<DT>(x[jt][0] * inv, x[jt][1] * inv, x[jt][2] * inv, x[jt][3] * inv);
#pragma unroll
      for (int dt = 0; dt < 2; ++dt) {
        f32x4_t o = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int jt = 0; jt < 4; ++jt) o = mma16<DT>(vt[dt][jt], p[jt], o);
        if (act && i < N)
          *(uint2*)(a.y + ((w * N + i) * a.heads + t.h) * 32 + dt * 16 + t.g * 4) = pack4<DT>(o[0], o[1], o[2], o[3]);
      }
      if (act && i < N && t.g == 0)
        *(float2*)(a.stat + ((w * a.heads + t.h) * N + i) * 2) = make_float2(m, l);
    }
    wa_lds_sync();  // the tile is rewritten by the next window
  }
}

template <int DT>
__global__ __launch_bounds__(256) void winattn_bwd_kernel(const WaArgs a, int slabs, int iters) {
  __shared__ __attribute__((aligned(16))) uint16_t ldsT[4][32 * kLd];  // dO^T, then Q^T, then K^T: [channel][token]
  __shared__ __attribute__((aligned(16))) uint16_t ldsP[4][64 * kLd];  // P, then dS: [key][query]
  const WaLane t = wa_lane(a.heads);
  const int N = a.N;
  uint16_t* T = ldsT[threadIdx.x >> 6];
  uint16_t* PS = ldsP[threadIdx.x >> 6];
  float bias[4][4][4], dbias[4][4][4];
  wa_bias(a.bias, t, N, bias);
#pragma unroll
  for (int it = 0; it < 4; ++it)
#pragma unroll
    for (int jt = 0; jt < 4; ++jt)
#pragma unroll
      for (int r = 0; r < 4; ++r) dbias[it][jt][r] = 0.f;
  const f32x4_t zero = {0.f, 0.f, 0.f, 0.f};

  for (int it0 = 0; it0 < iters; ++it0) {
    const int64_t w = t.slot + (int64_t)it0 * slabs;
    const bool act = w < a.Bw;
    uint4 qr[4], kr[4], vr[4], gr[4];
#pragma unroll
    for (int tt = 0; tt < 4; ++tt) {
      const int tok = tt * 16 + t.c;
      const bool ok = act && tok < N;
      qr[tt] = wa_row(a.q, w, t, tok, ok);
      kr[tt] = wa_row(a.k, w, t, tok, ok);
      vr[tt] = wa_row(a.v, w, t, tok, ok);
      gr[tt] = wa_row(a.dy, w, t, tok, ok);
    }
    int lq[4], lk[4][4];
    wa_labels(a.region, a.nwin, w, t, N, act, lq, lk);
    wa_put_t(T, gr, t);

    uint2 ds16[4][4];
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      const int i = it * 16 + t.c;
      const bool iok = act && i < N;
      f32x4_t s[4], dp[4];
#pragma unroll
      for (int jt = 0; jt < 4; ++jt) {
        s[jt] = mma32<DT>(kr[jt], qr[it], zero);
        dp[jt] = mma32<DT>(vr[jt], gr[it], zero);
      }
      float x[4][4];
      wa_scores(s, bias[it], lq[it], lk, t, N, a.scale, x);
      float2 ml = make_float2(0.f, 1.f);
      if (iok) ml = *(const float2*)(a.stat + ((w * a.heads + t.h) * N + i) * 2);
      const float inv = iok ? 1.f / ml.y : 0.f;  // rows past N: p = 0
      float D = 0.f;
#pragma unroll
      for (int jt = 0; jt < 4; ++jt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          x[jt][r] = __builtin_amdgcn_exp2f((x[jt][r] - ml.x) * kLog2e) * inv;
          D += x[jt][r] * dp[jt][r];
        }
      D = wa_qsum(D);
#pragma unroll
      for (int jt = 0; jt < 4; ++jt) {
        float d[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          d[r] = x[jt][r] * (dp[jt][r] - D);
          dbias[it][jt][r] += d[r];
          PS[(jt * 16 + t.g * 4 + r) * kLd + i] = E16<DT>::from_f(x[jt][r]);
        }
        ds16[it][jt] = pack4<DT>(d[0], d[1], d[2], d[3]);
      }
    }
    wa_lds_sync();
    // dV^T[d][j] = sum_i dO^T[d][i] P[i][j]
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
      for (int jt = 0; jt < 4; ++jt) {
        f32x4_t o = zero;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
          o = mma32<DT>(*(const uint4*)(T + (dt * 16 + t.c) * kLd + ks * 32 + t.g * 8),
                        *(const uint4*)(PS + (jt * 16 + t.c) * kLd + ks * 32 + t.g * 8), o);
        if (act && jt * 16 + t.c < N) wa_store4<DT>(a.dv, w, t, jt * 16 + t.c, dt, o, 1.f);
      }
    wa_lds_sync();
    wa_put_t(T, qr, t);
#pragma unroll
    for (int it = 0; it < 4; ++it)
#pragma unroll
      for (int jt = 0; jt < 4; ++jt) {
        const uint32_t lo = ds16[it][jt].x, hi = ds16[it][jt].y;
        const int col = it * 16 + t.c, row = jt * 16 + t.g * 4;
        PS[(row + 0) * kLd + col] = (uint16_t)lo;
        PS[(row + 1) * kLd + col] = (uint16_t)(lo >> 16);
        PS[(row + 2) * kLd + col] = (uint16_t)hi;
        PS[(row + 3) * kLd + col] = (uint16_t)(hi >> 16);
      }
    wa_lds_sync();
    // dK^T[d][j] = scale * sum_i Q^T[d][i] dS[i][j]
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
      for (int jt = 0; jt < 4; ++jt) {
        f32x4_t o = zero;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
          o = mma32<DT>(*(const uint4*)(T + (dt * 16 + t.c) * kLd + ks * 32 + t.g * 8),
                        *(const uint4*)(PS + (jt * 16 + t.c) * kLd + ks * 32 + t.g * 8), o);
        if (act && jt * 16 + t.c < N) wa_store4<DT>(a.dk, w, t, jt * 16 + t.c, dt, o, a.scale);
      }
    wa_lds_sync();
    wa_put_t(T, kr, t);
    wa_lds_sync();
    // dQ^T[d][i] = scale * sum_j K^T[d][j] dS^T[j][i]: dS from the registers
#pragma unroll
    for (int dt = 0; dt < 2; ++dt) {
      uint2 kt[4];
#pragma unroll
      for (int jt = 0; jt < 4; ++jt) kt[jt] = *(const uint2*)(T + (dt * 16 + t.c) * kLd + jt * 16 + t.g * 4);
#pragma unroll
      for (int it = 0; it < 4; ++it) {
        f32x4_t o = zero;
#pragma unroll
        for (int jt = 0; jt < 4; ++jt) o = mma16<DT>(kt[jt], ds16[it][jt], o);
        if (act && it * 16 + t.c < N) wa_store4<DT>(a.dq, w, t, it * 16 + t.c, dt, o, a.scale);
      }
    }
    wa_lds_sync();  // the tiles are rewritten by the next window
  }

  float* slab = a.partial + ((int64_t)t.slot * a.heads + t.h) * N * N;
#pragma unroll
  for (int it = 0; it < 4; ++it)
#pragma unroll
    for (int jt = 0; jt < 4; ++jt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = it * 16 + t.c, j = jt * 16 + t.g * 4 + r;
        if (i < N && j < N) slab[i * N + j] = dbias[it][jt][r];
      }
}

int gcd4(int h) { return h % 4 == 0 ? 4 : (h % 2 == 0 ? 2 : 1); }

void check_args(const char* what, int dtype, const WaArgs& a, const WaPlan& p) {
  if ((dtype != kBF16 && dtype != kF16) || !winattn_fits(a.Bw, a.heads, a.N, 32) || p.blocks < 1 || p.slabs < 1 ||
      (int64_t)p.blocks * 4 != (int64_t)p.slabs * a.heads || (a.region != nullptr && a.nwin < 1))
    pdt_hip_fail(what, hipErrorInvalidValue, __FILE__, __LINE__);
}

}  // namespace

bool winattn_fits(int64_t Bw, int64_t heads, int64_t N, int64_t head_dim) {
  return head_dim == 32 && N >= 1 && N <= 64 && heads >= 1 && heads <= 256 && Bw >= 1 && Bw < (int64_t(1) << 31) &&
         Bw * heads * N * 96 < (int64_t(1) << 40);
}

WaPlan winattn_plan(int64_t Bw, int heads, int max_blocks) {
  const int64_t unit = heads / gcd4(heads);  // blocks * 4 must be a multiple of heads
  int64_t want = (Bw * heads + 3) / 4;       // one (window, head) per wave
  if (want > max_blocks) want = max_blocks;
  int64_t blocks = want / unit * unit;
  if (blocks < unit) blocks = unit;
  return WaPlan{(int)blocks, (int)(blocks * 4 / heads)};
}

void winattn_fwd_launch(int dtype, const WaArgs& a, const WaPlan& plan, hipStream_t s) {
  check_args("winattn_fwd_launch: arguments outside the kernels' contract", dtype, a, plan);
  PDT_COUNT("winattn_fwd");
  const int iters = (int)((a.Bw + plan.slabs - 1) / plan.slabs);
  if (dtype == kBF16)
    hipLaunchKernelGGL((winattn_fwd_kernel<kBF16>), dim3((unsigned)plan.blocks), dim3(256), 0, s, a, plan.slabs, iters);
  else
    hipLaunchKernelGGL((winattn_fwd_kernel<kF16>), dim3((unsigned)plan.blocks), dim3(256), 0, s, a, plan.slabs, iters);
}

void winattn_bwd_launch(int dtype, const WaArgs& a, const WaPlan& plan, hipStream_t s) {
  check_args("winattn_bwd_launch: arguments outside the kernels' contract", dtype, a, plan);
  PDT_COUNT("winattn_bwd");
  const int iters = (int)((a.Bw + plan.slabs - 1) / plan.slabs);
  if (dtype == kBF16)
    hipLaunchKernelGGL((winattn_bwd_kernel<kBF16>), dim3((unsigned)plan.blocks), dim3(256), 0, s, a, plan.slabs, iters);
  else
    hipLaunchKernelGGL((winattn_bwd_kernel<kF16>), dim3((unsigned)plan.blocks), dim3(256), 0, s, a, plan.slabs, iters);
}

}  // namespace pdt
