// Global multi-head attention for the torch engine (SURVEY §2.2 model registry: every ViT encoder block):
//   y = softmax(scale * q k^T) v
// per (batch, head) over N <= 4096 tokens, heads of dimension 64, 16-bit operands, fp32 math.  The sequence does not fit
// a wave's registers: every kernel loops over 64-token blocks of the operand it does not own, the forward with a
// running max and sum (online softmax), the backward with P recomputed from the saved log-sum-exp.
//
// Work split (all three kernels): a block is 4 waves and owns 128 tokens of one (batch, head); wave w owns the 16-token
// tiles w and w + 4 of them (so a 50-token sequence still uses all four waves) and skips a tile that starts past N.
// Blocks of one (batch, head) are adjacent in the grid: after the first, the other side's blocks come from L2.  The
// 64-token block of the looped-over operands is staged ONCE per block into LDS as [token][64 ch] rows of 160 bytes
// (16-byte writes; 8 rows of a transposed read fall on 8 distinct 32-byte bank groups) and every wave reads its MFMA
// operands from there.  Lane l = 16 g + c.
//   * forward: S^T = K Q^T with v_mfma_f32_16x16x32, two K steps over the 64 channels: A = K rows from LDS (lane: key
//     16 jt + c, channels 32 ks + 8 g ..), B = Q rows held in registers.  The four accumulators of tile jt are the keys
//     16 jt + 4 g + r of query c: a query's 64 keys of the block sit in 4 lanes, so block max and block sum are an
//     in-lane pass and two xor steps.  Per query a running max m and sum l (base-2 domain: scores are scaled by
//     scale * log2 e once); p = exp2(x - m) is rounded UNNORMALISED and is the B operand of O^T += V^T P^T as it
//     stands: two key tiles jt = 2 jp, 2 jp + 1 pair into one 16x16x32 (k slot 8 g + e is key 32 jp + 16 (e / 4) + 4 g
//     + e % 4), and A = V^T comes from the row-major LDS image through the transposing read ds_read_b64_tr_b16 (no
//     2-byte LDS writes anywhere).  The 4 channel tiles of O^T are scaled by exp2(m_old - m_new) every block (1 exactly
//     when the max did not move); the one division by l happens at the end.  lse = m + log2 l, base 2.
//   * backward, deterministic, no atomics: two passes that each recompute S^T and dP^T = V dO^T, so 7 matrix products
//     (S, dP, dQ | S, dP, dV, dK) where a single pass with atomic dQ needs 5 -- the price of bit-identical runs.
//       - mha_bwd_dq_kernel owns queries, loops over key blocks: p = exp2(x - lse), dS = p (dP - delta),
//         dQ^T += K^T dS^T with dS from registers (paired as P is in the forward) and K^T by the transposing read.
//         It also forms delta_i = sum_d dO_id y_id for its rows -- as the diagonal of the MFMA product Y dO^T, i.e. by
//         the very instruction sequence that forms dP, so a one-token sequence (y == v) gets dS == 0 exactly -- and
//         writes it to the fp32 workspace the second pass reads.
//       - mha_bwd_dkv_kernel owns keys (K, V rows in registers as the A operands), loops over query blocks (Q, dO
//         staged).  dV^T = dO^T P and dK^T = Q^T dS contract over queries, which lie across lanes: each wave writes
//         its rounded P and dS tiles to a private LDS image [query][32 keys] (8-byte writes: 4 keys of one query) and
//         both operands of the 16x16x32 MFMA come back through transposing reads (dO^T / Q^T from the staged blocks).
//     All outputs: 4 channels of one token per lane, 8-byte stores.
// Keys >= N get -inf before the max (p = 0 exactly).  Rows >= N are staged / loaded as zeros and never stored; in the
// backward they read lse = +inf, so p = 0 and they add nothing to dK or dV.
#include <math.h>

#include "../common.h"
#include "mha.h"

namespace pdt {

namespace {

constexpr int kLd = 80;   // 16-bit elements per row of a staged [token][64 ch] image (160 bytes)
constexpr int kLp = 40;   // per row of a wave's [query][32 keys] P / dS image (80 bytes)
constexpr int kT = 2;     // 16-token tiles a wave owns
constexpr int kOwn = 128; // tokens a block owns: 4 waves * kT * 16
constexpr float kLog2e = 1.4426950408889634f;

typedef __attribute__((address_space(3))) s16x4_t mh_lds_s16x4;

// v_mfma_f32_16x16x32: A[m = c][k = 8 g + e], B[k = 8 g + e][n = c], D[m = 4 g + r][n = c]
template <int DT>
PDT_DEVICE f32x4_t mma32(uint4 a, uint4 b, f32x4_t acc) {
  using V = typename E16<DT>::vec8;
  return E16<DT>::mfma16x16x32(__builtin_bit_cast(V, a), __builtin_bit_cast(V, b), acc);
}

// both K steps over the 64 channels
template <int DT>
PDT_DEVICE f32x4_t mma64(const uint4 (&a)[2], const uint4 (&b)[2]) {
  return mma32<DT>(a[1], b[1], mma32<DT>(a[0], b[0], f32x4_t{0.f, 0.f, 0.f, 0.f}));
}

template <int DT>
PDT_DEVICE uint2 pack4(f32x4_t v) {
  return make_uint2(E16<DT>::pack2(v[0], v[1]), E16<DT>::pack2(v[2], v[3]));
}

struct MhLane {
  int c, g, q4, p4, wave, h, chunk;
  int64_t b;
  // first token of the wave's tile i
  PDT_DEVICE int tile0(int i) const { return chunk * kOwn + (wave + 4 * i) * 16; }
};

PDT_DEVICE MhLane mh_lane(int heads, int chunks) {
  const int lane = threadIdx.x & 63, bh = (int)blockIdx.x / chunks;
  return MhLane{lane & 15, lane >> 4, (lane & 15) >> 2, lane & 3, (int)threadIdx.x >> 6, bh % heads,
                (int)blockIdx.x % chunks, bh / heads};
}

PDT_DEVICE uint16_t* mh_at(const WaOperand& o, const MhLane& t, int tok) {
  return o.p + t.b * o.sw + (int64_t)tok * o.st + (int64_t)t.h * o.sh;
}

// channels 32 ks + 8 g .. + 7 of token `tok`, ks = 0, 1 (zeros when !ok): a B operand, or an A operand of the owner
PDT_DEVICE void mh_rows(const WaOperand& o, const MhLane& t, int tok, bool ok, uint4 (&r)[2]) {
#pragma unroll
  for (int ks = 0; ks < 2; ++ks)
    r[ks] = ok ? *(const uint4*)(mh_at(o, t, tok) + ks * 32 + t.g * 8) : make_uint4(0u, 0u, 0u, 0u);
}

// tokens t0 .. t0 + 63 of an operand into the row-major LDS image (zeros past N): 512 16-byte chunks, two per thread
PDT_DEVICE void mh_stage(uint16_t* img, const WaOperand& o, const MhLane& t, int t0, int N) {
  const int row = (int)threadIdx.x >> 3, ch = (int)threadIdx.x & 7;
  uint4 v[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int tok = t0 + row + 32 * j;
    v[j] = tok < N ? *(const uint4*)(mh_at(o, t, tok) + ch * 8) : make_uint4(0u, 0u, 0u, 0u);
  }
#pragma unroll
  for (int j = 0; j < 2; ++j) *(uint4*)(img + (row + 32 * j) * kLd + ch * 8) = v[j];
}

// the row-major operand of a staged image: token 16 tt + c, channels 32 ks + 8 g ..
PDT_DEVICE void mh_frag(const uint16_t* img, const MhLane& t, int tt, uint4 (&r)[2]) {
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) r[ks] = *(const uint4*)(img + (tt * 16 + t.c) * kLd + ks * 32 + t.g * 8);
}

// Transposed operand from a row-major image with `ld` elements per row: the lane receives column col0 + c of the rows
// lo .. lo + 3 (k slots 8 g + 0..3) and hi .. hi + 3 (k slots 8 g + 4..7).  ds_read_b64_tr_b16: within 16 lanes, lane
// 4 q4 + p4 names 4 elements of one row, and lane c gets element c of each of the 4 rows.
PDT_DEVICE uint4 mh_tr(const uint16_t* img, int ld, const MhLane& t, int lo, int hi, int col0) {
  const s16x4_t a = __builtin_amdgcn_ds_read_tr16_b64_v4i16((mh_lds_s16x4*)(img + (lo + t.q4) * ld + col0 + 4 * t.p4));
  const s16x4_t b = __builtin_amdgcn_ds_read_tr16_b64_v4i16((mh_lds_s16x4*)(img + (hi + t.q4) * ld + col0 + 4 * t.p4));
  return __builtin_bit_cast(uint4, __builtin_shufflevector(a, b, 0, 1, 2, 3, 4, 5, 6, 7));
}

// the transposed [64 ch][key pair jp] operands of a staged block for the products that contract over its tokens with
// the other operand in registers: k slot 8 g + e is token 32 jp + 16 (e / 4) + 4 g + e % 4
PDT_DEVICE void mh_tr_paired(const uint16_t* img, const MhLane& t, uint4 (&f)[4][2]) {
#pragma unroll
  for (int dt = 0; dt < 4; ++dt)
#pragma unroll
    for (int jp = 0; jp < 2; ++jp) f[dt][jp] = mh_tr(img, kLd, t, jp * 32 + t.g * 4, jp * 32 + 16 + t.g * 4, dt * 16);
}

// 4 channels 16 dt + 4 g .. of token `tok`, scaled and rounded once
template <int DT>
PDT_DEVICE void mh_store4(uint16_t* at, const MhLane& t, int dt, f32x4_t v, float scale) {
  *(uint2*)(at + dt * 16 + t.g * 4) = pack4<DT>(v * scale);
}

// over the 4 lanes (c, g = 0..3) that share a query
PDT_DEVICE float mh_qmax(float v) {
  v = fmaxf(v, __shfl_xor(v, 16, 64));
  return fmaxf(v, __shfl_xor(v, 32, 64));
}
PDT_DEVICE float mh_qsum(float v) {
  v += __shfl_xor(v, 16, 64);
  return v + __shfl_xor(v, 32, 64);
}

template <int DT>
__global__ __launch_bounds__(256) void mha_fwd_kernel(const MhaArgs a, int chunks) {
  __shared__ __attribute__((aligned(16))) uint16_t Ks[64 * kLd];
  __shared__ __attribute__((aligned(16))) uint16_t Vs[64 * kLd];
  const MhLane t = mh_lane(a.heads, chunks);
  const int N = a.N;
  const float sc2 = a.scale * kLog2e;
  const f32x4_t zero = {0.f, 0.f, 0.f, 0.f};

  uint4 qr[kT][2];
  float m[kT], l[kT];
  f32x4_t o[kT][4];
#pragma unroll
  for (int i = 0; i < kT; ++i) {
    const int row = t.tile0(i) + t.c;
    mh_rows(a.q, t, row, row < N, qr[i]);
    m[i] = -INFINITY;
    l[i] = 0.f;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) o[i][dt] = zero;
  }

  for (int k0 = 0; k0 < N; k0 += 64) {
    __syncthreads();  // the previous block's reads
    mh_stage(Ks, a.k, t, k0, N);
    mh_stage(Vs, a.v, t, k0, N);
    __syncthreads();
    uint4 kf[4][2], vt[4][2];
#pragma unroll
    for (int jt = 0; jt < 4; ++jt) mh_frag(Ks, t, jt, kf[jt]);
    mh_tr_paired(Vs, t, vt);
#pragma unroll
    for (int i = 0; i < kT; ++i) {
      if (t.tile0(i) >= N) continue;  // wave-uniform
      f32x4_t x[4];
      float mx = m[i];
#pragma unroll
      for (int jt = 0; jt < 4; ++jt) {
        x[jt] = mma64<DT>(kf[jt], qr[i]);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          x[jt][r] = (k0 + jt * 16 + t.g * 4 + r < N) ? x[jt][r] * sc2 : -INFINITY;
          mx = fmaxf(mx, x[jt][r]);
        }
      }
      mx = mh_qmax(mx);  // key k0 is always real: mx is finite
      const float alpha = __builtin_amdgcn_exp2f(m[i] - mx);
      m[i] = mx;
      float sum = 0.f;
#pragma unroll
      for (int jt = 0; jt < 4; ++jt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          x[jt][r] = __builtin_amdgcn_exp2f(x[jt][r] - mx);
          sum += x[jt][r];
        }
      l[i] = l[i] * alpha + mh_qsum(sum);
#pragma unroll
      for (int jp = 0; jp < 2; ++jp) {
        const uint2 lo = pack4<DT>(x[2 * jp]), hi = pack4<DT>(x[2 * jp + 1]);
        const uint4 p = make_uint4(lo.x, lo.y, hi.x, hi.y);
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
          if (jp == 0) o[i][dt] = o[i][dt] * alpha;
          o[i][dt] = mma32<DT>(vt[dt][jp], p, o[i][dt]);
        }
      }
    }
  }

#pragma unroll
  for (int i = 0; i < kT; ++i) {
    const int row = t.tile0(i) + t.c;
    if (row >= N) continue;
    const float inv = 1.f / l[i];
    uint16_t* y = a.y + ((t.b * N + row) * a.heads + t.h) * 64;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) mh_store4<DT>(y, t, dt, o[i][dt], inv);
    if (t.g == 0) a.lse[(t.b * a.heads + t.h) * N + row] = m[i] + log2f(l[i]);
  }
}

// p = exp2(x * sc2 - lse) and dS = p (dP - delta) of one S^T / dP^T tile pair, in place: s <- p, dp <- dS
PDT_DEVICE void mh_p_ds(f32x4_t& s, f32x4_t& dp, float sc2, float lse, float delta) {
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    s[r] = __builtin_amdgcn_exp2f(s[r] * sc2 - lse);
    dp[r] = s[r] * (dp[r] - delta);
  }
}

template <int DT>
__global__ __launch_bounds__(256) void mha_bwd_dq_kernel(const MhaArgs a, int chunks) {
  __shared__ __attribute__((aligned(16))) uint16_t Ks[64 * kLd];
  __shared__ __attribute__((aligned(16))) uint16_t Vs[64 * kLd];
  const MhLane t = mh_lane(a.heads, chunks);
  const int N = a.N;
  const float sc2 = a.scale * kLog2e;
  const f32x4_t zero = {0.f, 0.f, 0.f, 0.f};
  const WaOperand yo = {a.y, (int64_t)N * a.heads * 64, (int64_t)a.heads * 64, 64};

  uint4 qr[kT][2], gr[kT][2];
  float lse[kT], delta[kT];
  f32x4_t dq[kT][4];
#pragma unroll
  for (int i = 0; i < kT; ++i) {
    const int row = t.tile0(i) + t.c;
    const bool ok = row < N;
    uint4 yr[2];
    mh_rows(a.q, t, row, ok, qr[i]);
    mh_rows(a.dy, t, row, ok, gr[i]);
    mh_rows(yo, t, row, ok, yr);
    // delta: the diagonal of Y dO^T; element (m = 4 g + r, n = c) is the diagonal one where 4 g + r == c
    const f32x4_t d = mma64<DT>(yr, gr[i]);
    const int r = t.c & 3;
    const float pick = r == 0 ? d[0] : r == 1 ? d[1] : r == 2 ? d[2] : d[3];
    delta[i] = mh_qsum(t.g == (t.c >> 2) ? pick : 0.f);
    const int64_t at = (t.b * a.heads + t.h) * N + row;
    lse[i] = ok ? a.lse[at] : INFINITY;
    if (ok && t.g == 0) a.delta[at] = delta[i];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) dq[i][dt] = zero;
  }

  for (int k0 = 0; k0 < N; k0 += 64) {
    __syncthreads();
    mh_stage(Ks, a.k, t, k0, N);
    mh_stage(Vs, a.v, t, k0, N);
    __syncthreads();
    uint4 kf[4][2], vf[4][2], kt[4][2];
#pragma unroll
    for (int jt = 0; jt < 4; ++jt) {
      mh_frag(Ks, t, jt, kf[jt]);
      mh_frag(Vs, t, jt, vf[jt]);
    }
    mh_tr_paired(Ks, t, kt);
#pragma unroll
    for (int i = 0; i < kT; ++i) {
      if (t.tile0(i) >= N) continue;  // wave-uniform
      uint2 ds[4];
#pragma unroll
      for (int jt = 0; jt < 4; ++jt) {
        f32x4_t s = mma64<DT>(kf[jt], qr[i]), dp = mma64<DT>(vf[jt], gr[i]);
        mh_p_ds(s, dp, sc2, lse[i], delta[i]);
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (k0 + jt * 16 + t.g * 4 + r >= N) dp[r] = 0.f;
        ds[jt] = pack4<DT>(dp);
      }
#pragma unroll
      for (int jp = 0; jp < 2; ++jp) {
        const uint4 b = make_uint4(ds[2 * jp].x, ds[2 * jp].y, ds[2 * jp + 1].x, ds[2 * jp + 1].y);
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) dq[i][dt] = mma32<DT>(kt[dt][jp], b, dq[i][dt]);
      }
    }
  }

#pragma unroll
  for (int i = 0; i < kT; ++i) {
    const int row = t.tile0(i) + t.c;
    if (row >= N) continue;
    uint16_t* at = mh_at(a.dq, t, row);
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) mh_store4<DT>(at, t, dt, dq[i][dt], a.scale);
  }
}

template <int DT>
__global__ __launch_bounds__(256) void mha_bwd_dkv_kernel(const MhaArgs a, int chunks) {
  __shared__ __attribute__((aligned(16))) uint16_t Qs[64 * kLd];
  __shared__ __attribute__((aligned(16))) uint16_t Gs[64 * kLd];
  __shared__ __attribute__((aligned(16))) uint16_t Ps[4][64 * kLp];  // per wave: rounded P [query][16 i + key]
  __shared__ __attribute__((aligned(16))) uint16_t Ds[4][64 * kLp];  // per wave: rounded dS
  const MhLane t = mh_lane(a.heads, chunks);
  const int N = a.N;
  const float sc2 = a.scale * kLog2e;
  const f32x4_t zero = {0.f, 0.f, 0.f, 0.f};
  uint16_t* P = Ps[t.wave];
  uint16_t* D = Ds[t.wave];

  uint4 kr[kT][2], vr[kT][2];
  f32x4_t dk[kT][4], dv[kT][4];
#pragma unroll
  for (int i = 0; i < kT; ++i) {
    const int row = t.tile0(i) + t.c;
    mh_rows(a.k, t, row, row < N, kr[i]);
    mh_rows(a.v, t, row, row < N, vr[i]);
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) dk[i][dt] = dv[i][dt] = zero;
  }

  for (int q0 = 0; q0 < N; q0 += 64) {
    __syncthreads();  // the previous block's reads of all four images
    mh_stage(Qs, a.q, t, q0, N);
    mh_stage(Gs, a.dy, t, q0, N);
    float lse[4], delta[4];
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      const int row = q0 + it * 16 + t.c;
      const int64_t at = (t.b * a.heads + t.h) * N + row;
      lse[it] = row < N ? a.lse[at] : INFINITY;  // rows past N: p = 0
      delta[it] = row < N ? a.delta[at] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      uint4 qf[2], gf[2];
      mh_frag(Qs, t, it, qf);
      mh_frag(Gs, t, it, gf);
#pragma unroll
      for (int i = 0; i < kT; ++i) {
        if (t.tile0(i) >= N) continue;  // wave-uniform
        f32x4_t s = mma64<DT>(kr[i], qf), dp = mma64<DT>(vr[i], gf);  // keys 4 g + r of tile i, query 16 it + c
        mh_p_ds(s, dp, sc2, lse[it], delta[it]);
        *(uint2*)(P + (it * 16 + t.c) * kLp + i * 16 + t.g * 4) = pack4<DT>(s);
        *(uint2*)(D + (it * 16 + t.c) * kLp + i * 16 + t.g * 4) = pack4<DT>(dp);
      }
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {  // queries 32 kk + 8 g + e are the k slots
      const int lo = kk * 32 + t.g * 8, hi = lo + 4;
      uint4 gt[4], qt[4];
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) {
        gt[dt] = mh_tr(Gs, kLd, t, lo, hi, dt * 16);
        qt[dt] = mh_tr(Qs, kLd, t, lo, hi, dt * 16);
      }
#pragma unroll
      for (int i = 0; i < kT; ++i) {
        if (t.tile0(i) >= N) continue;
        const uint4 pb = mh_tr(P, kLp, t, lo, hi, i * 16), db = mh_tr(D, kLp, t, lo, hi, i * 16);
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
          dv[i][dt] = mma32<DT>(gt[dt], pb, dv[i][dt]);  // dV^T[d][j] += sum_i dO^T[d][i] P[i][j]
          dk[i][dt] = mma32<DT>(qt[dt], db, dk[i][dt]);  // dK^T[d][j] += sum_i Q^T[d][i] dS[i][j]
        }
      }
    }
  }

#pragma unroll
  for (int i = 0; i < kT; ++i) {
    const int row = t.tile0(i) + t.c;
    if (row >= N) continue;
    uint16_t* atk = mh_at(a.dk, t, row);
    uint16_t* atv = mh_at(a.dv, t, row);
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
      mh_store4<DT>(atk, t, dt, dk[i][dt], a.scale);
      mh_store4<DT>(atv, t, dt, dv[i][dt], 1.f);
    }
  }
}

int mh_chunks(int N) { return (N + kOwn - 1) / kOwn; }

void check_args(const char* what, int dtype, const MhaArgs& a) {
  if ((dtype != kBF16 && dtype != kF16) || !mha_fits(a.B, a.heads, a.N, 64) || a.lse == nullptr || a.y == nullptr)
    pdt_hip_fail(what, hipErrorInvalidValue, __FILE__, __LINE__);
}

}  // namespace

bool mha_fits(int64_t B, int64_t heads, int64_t N, int64_t head_dim) {
  return head_dim == 64 && N >= 1 && N <= 4096 && heads >= 1 && heads <= 256 && B >= 1 && B < (int64_t(1) << 31) &&
         B * heads * ((N + kOwn - 1) / kOwn) < (int64_t(1) << 31) && B * heads * N * 192 < (int64_t(1) << 40);
}

void mha_fwd_launch(int dtype, const MhaArgs& a, hipStream_t s) {
  check_args("mha_fwd_launch: arguments outside the kernels' contract", dtype, a);
  PDT_COUNT("mha_fwd");
  const int chunks = mh_chunks(a.N);
  const dim3 grid((unsigned)(a.B * a.heads * chunks));
  if (dtype == kBF16)
    hipLaunchKernelGGL((mha_fwd_kernel<kBF16>), grid, dim3(256), 0, s, a, chunks);
  else
    hipLaunchKernelGGL((mha_fwd_kernel<kF16>), grid, dim3(256), 0, s, a, chunks);
}

void mha_bwd_launch(int dtype, const MhaArgs& a, hipStream_t s) {
  check_args("mha_bwd_launch: arguments outside the kernels' contract", dtype, a);
  if (a.delta == nullptr) pdt_hip_fail("mha_bwd_launch: no delta workspace", hipErrorInvalidValue, __FILE__, __LINE__);
  PDT_COUNT("mha_bwd");
  const int chunks = mh_chunks(a.N);
  const dim3 grid((unsigned)(a.B * a.heads * chunks));
  if (dtype == kBF16) {
    hipLaunchKernelGGL((mha_bwd_dq_kernel<kBF16>), grid, dim3(256), 0, s, a, chunks);
    hipLaunchKernelGGL((mha_bwd_dkv_kernel<kBF16>), grid, dim3(256), 0, s, a, chunks);
  } else {
    hipLaunchKernelGGL((mha_bwd_dq_kernel<kF16>), grid, dim3(256), 0, s, a, chunks);
    hipLaunchKernelGGL((mha_bwd_dkv_kernel<kF16>), grid, dim3(256), 0, s, a, chunks);
  }
}

}  // namespace pdt
