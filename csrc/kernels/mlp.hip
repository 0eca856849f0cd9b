// The second Linear of a channel MLP with everything around it folded in (mlp.h): z0 = round16(x * w1^T) comes from
// pwconv.hip, and the bias b1, the exact GELU, its derivative and the bias b2 live in the three GEMMs that touch the
// hidden tensor [M][Hd], which is therefore read twice less in the forward and five times less in the backward than
// by separate ops, and only z0 is kept.  v_mfma_f32_16x16x32_{bf16,f16}, fp32 accumulation, wave64, no atomics.
//
//   * mlp_fc2_fwd_kernel: y[M][Co] = gelu(z0 + b1) * w2^T + b2, a LONG reduction (Hd = 4C up to 2048), the case
//     pwconv_gemm_kernel is weak at (per-wave weight fragments from L2 every step).  A persistent block (4 waves) owns
//     one column block of NB = 128 or 256 output channels and walks 64-row tiles.  Per reduction step of BK hidden
//     channels the block's 256 threads load the [64][BK] z0 tile ONCE (16-byte loads), add b1, apply GELU in
//     registers and write the rounded h tile to LDS next to the [NB][BK] w2 tile; both are double-buffered, the next
//     step's global loads are in flight behind this step's MFMAs.  The waves split the block's channels (NB / 4 each)
//     and all read the same h tile.  Rows of both LDS images are BK * 2 bytes with the 16-byte chunks XOR-swizzled by
//     row, so the 16 rows a ds_read_b128 fragment load touches spread over the banks.  The weights are the MFMA A
//     operand in pwconv.hip's fragment-row permutation: a lane ends with 8 consecutive channels of one row, adds b2 and
//     stores 16 bytes.
//   * mlp_fc2_dgrad_kernel: dz[M][Hd] = (dy * w2t^T) .* gelu'(z0 + b1), a SHORT reduction (Co <= 512): operands straight
//     from memory in the MFMA layout as in pwconv_gemm_kernel (no LDS), next step's fragments behind this step's MFMAs.
//     The epilogue loads the lane's 16 bytes of z0, multiplies by gelu', rounds, stores, and adds the ROUNDED values to
//     the lane's fp32 column sums, kept across every tile the block walks; 16 lanes are folded by DPP, the 4 waves
//     through LDS in wave order, and the block writes its slice of one partial row (col_reduce.h's [blocks][C][1]).
//   * mlp_fc2_wgrad_kernel: dw2[Co][Hd] = dy^T * h split over M into fp32 slabs, pwconv_wgrad_kernel's LDS image and
//     transposed reads; the z0 tile becomes h (b1, GELU, rounding) on its way from registers into the image.
//
// Tails are masked at the load (rows past M, 16-byte chunks past Hd / Co, weight rows past the width -> kOOB, zeros;
// a masked h chunk is written as zeros, never as gelu(b1)) and dropped at the store.  Operands are addressed through
// per-tile buffer resources (64-bit tile base, small offsets): their byte size is not limited.
#include "../common.h"
#include "conv_wgrad.h"
#include "mlp.h"

namespace pdt {

namespace {

typedef unsigned int ml_v4u __attribute__((vector_size(16)));
typedef __attribute__((address_space(3))) s16x4_t ml_lds_s16x4;

PDT_DEVICE uint4 ml_load16(__amdgpu_buffer_rsrc_t r, uint32_t off) {
  return __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(r, (int)off, 0, 0));
}
PDT_DEVICE void ml_store16(__amdgpu_buffer_rsrc_t r, uint32_t off, uint4 v) {
  __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(ml_v4u, v), r, (int)off, 0, 0);
}
// a + b, or kOOB when either part is kOOB
PDT_DEVICE uint32_t ml_off(uint32_t a, uint32_t b) { return ((a | b) & kOOB) ? kOOB : a + b; }
// pwconv.hip's fragment-row permutation: fragments 2p and 2p + 1 give a lane (rows 4 * fq + r) the 8 consecutive
// channels p * 32 + 8 * fq + [0, 8)
PDT_DEVICE int ml_frag_ch(int i, int row) { return (i >> 1) * 32 + (row >> 2) * 8 + (i & 1) * 4 + (row & 3); }

template <int CTRL>
PDT_DEVICE float ml_dpp(float x) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), CTRL, 0xf, 0xf, false));
}
// sum over the 16 lanes of a DPP row in a fixed butterfly: every lane ends with the same total
PDT_DEVICE float ml_row16_fold(float v) {
  v += ml_dpp<0xB1>(v);   // quad_perm [1, 0, 3, 2]
  v += ml_dpp<0x4E>(v);   // quad_perm [2, 3, 0, 1]
  v += ml_dpp<0x141>(v);  // row_half_mirror
  v += ml_dpp<0x140>(v);  // row_mirror
  return v;
}

// ---- the one GELU and the one derivative of the three kernels: exact (erf) form, fp32
PDT_DEVICE float mlp_gelu(float v) { return 0.5f * v * (1.f + erff(v * 0.70710678118654752f)); }
// gelu'(v) = Phi(v) + v * phi(v)
PDT_DEVICE float mlp_gelu_grad(float v) {
  const float cdf = 0.5f * (1.f + erff(v * 0.70710678118654752f));
  const float pdf = 0.39894228040143268f * expf(-0.5f * v * v);
  return cdf + v * pdf;
}

// b1[k .. k + 8) for a chunk wholly inside the width n (widths are multiples of 8), zeros for one outside; scalar loads:
// a parameter may sit anywhere in a flattened buffer
PDT_DEVICE void ml_bias8(const float* __restrict__ b, int k, int n, float (&o)[8]) {
#pragma unroll
  for (int e = 0; e < 8; ++e) o[e] = k < n ? b[k + e] : 0.f;
}

// a 16-byte chunk of z0 -> the chunk of h = round16(gelu(z0 + b1)); a masked chunk (`ok` false) is zeros
template <int DT>
PDT_DEVICE uint4 mlp_act8(uint4 z, const float (&b)[8], bool ok) {
  using E = E16<DT>;
  uint16_t e[8];
  unpack8(z, e);
  uint32_t w[4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
    w[i] = E::pack2(mlp_gelu(E::to_f(e[2 * i]) + b[2 * i]), mlp_gelu(E::to_f(e[2 * i + 1]) + b[2 * i + 1]));
  return ok ? make_uint4(w[0], w[1], w[2], w[3]) : make_uint4(0u, 0u, 0u, 0u);
}

// chunk swizzle of a [row][BK] LDS image read by rows (ds_read_b128 of chunk c of 16 consecutive rows)
template <int BK>
PDT_DEVICE int ml_swz(int row) { return BK == 64 ? (row & 7) : ((row >> 1) & 3); }

// ------------------------------------------------------------------------------------------------ forward
// NGW: 32-channel group pairs per wave (the block's column block is NB = 4 * NGW * 32 channels); BK: hidden channels
// per reduction step.  Grid: column block = blockIdx.x % ncb (neighbours share a z0 tile through L2).
template <int DT, int NGW, int BK>
__global__ __launch_bounds__(256) void mlp_fc2_fwd_kernel(const uint16_t* __restrict__ z0, const float* __restrict__ b1,
                                                          const uint16_t* __restrict__ w2, const float* __restrict__ b2,
                                                          uint16_t* __restrict__ y, int64_t M, int Hd, int Co, int ncb,
                                                          int mtiles) {
  using E = E16<DT>;
  typedef typename E::vec8 vec8;
  constexpr int BR = 64, PT = BR / 16;  // rows per tile, row fragments
  constexpr int NF = 2 * NGW;           // 16-channel weight fragments per wave
  constexpr int NB = 4 * NGW * 32;      // channels per column block
  constexpr int KC = BK / 8;            // 16-byte chunks per LDS row
  constexpr int ROWB = BK * 2;
  constexpr int NZ = BR * KC / 256, NW = NB * KC / 256;  // chunks a thread stages per step
  constexpr int HB = BR * ROWB, STAGE = HB + NB * ROWB;
  static_assert(NZ >= 1 && NW >= 1 && 2 * STAGE <= 65536, "tile shape");
  __shared__ __attribute__((aligned(16))) char smem[2 * STAGE];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int fr = lane & 15, fq = lane >> 4;
  const int cb = blockIdx.x % ncb;
  const int n0 = cb * NB;             // the block's first channel
  const int wn0 = wave * NGW * 32;    // the wave's first channel within the block
  const int tstride = gridDim.x / ncb;  // the launcher's grid is a multiple of ncb
  const int nsteps = (Hd + BK - 1) / BK;
  const __amdgpu_buffer_rsrc_t rw = make_rsrc(w2, (uint32_t)Co * (uint32_t)Hd * 2u);  // <= 2 MiB

  // a 32-channel group wholly past Co is skipped (wave-uniform)
  bool gok[NGW];
#pragma unroll
  for (int p = 0; p < NGW; ++p) gok[p] = n0 + wn0 + p * 32 < Co;

  // staging geometry, the same every step: chunk (row, ch) of the image goes to row * ROWB + ((ch ^ swz(row)) << 4)
  int zrow[NZ], zch[NZ], zlds[NZ];
#pragma unroll
  for (int q = 0; q < NZ; ++q) {
    const int idx = q * 256 + tid;
    zrow[q] = idx / KC;
    zch[q] = idx % KC;
    zlds[q] = zrow[q] * ROWB + ((zch[q] ^ ml_swz<BK>(zrow[q])) << 4);
  }
  int wch[NW], wlds[NW];
  uint32_t wrowoff[NW];  // byte offset of the weight row, kOOB past Co
#pragma unroll
  for (int q = 0; q < NW; ++q) {
    const int idx = q * 256 + tid;
    const int row = idx / KC;
    wch[q] = idx % KC;
    wlds[q] = HB + row * ROWB + ((wch[q] ^ ml_swz<BK>(row)) << 4);
    wrowoff[q] = n0 + row < Co ? (uint32_t)(n0 + row) * (uint32_t)Hd * 2u : kOOB;
  }

  float bo[NGW][8];  // b2 of the lane's 8 channels per group
#pragma unroll
  for (int p = 0; p < NGW; ++p) ml_bias8(b2, n0 + wn0 + p * 32 + 8 * fq, Co, bo[p]);

  uint4 rz[NZ], rwv[NW];
  float rb[NZ][8];
  bool zok[NZ];

  for (int t = blockIdx.x / ncb; t < mtiles; t += tstride) {
    const int64_t m0 = (int64_t)t * BR;
    const int64_t left = M - m0;
    const int rows = left < BR ? (int)left : BR;
    const __amdgpu_buffer_rsrc_t ri = make_rsrc(z0 + m0 * Hd, (uint32_t)rows * (uint32_t)Hd * 2u);
    const __amdgpu_buffer_rsrc_t ro = make_rsrc(y + m0 * Co, (uint32_t)rows * (uint32_t)Co * 2u);

    auto gload = [&](int step) {
#pragma unroll
      for (int q = 0; q < NZ; ++q) {
        const int k = step * BK + zch[q] * 8;
        zok[q] = k < Hd && zrow[q] < rows;
        rz[q] = ml_load16(ri, zok[q] ? ((uint32_t)zrow[q] * (uint32_t)Hd + (uint32_t)k) * 2u : kOOB);
        ml_bias8(b1, k, Hd, rb[q]);
      }
#pragma unroll
      for (int q = 0; q < NW; ++q) {
        const int k = step * BK + wch[q] * 8;
        rwv[q] = ml_load16(rw, ml_off(wrowoff[q], k < Hd ? (uint32_t)k * 2u : kOOB));
      }
    };
    auto lstore = [&](int buf) {
      char* sb = smem + buf * STAGE;
#pragma unroll
      for (int q = 0; q < NZ; ++q) *(uint4*)(sb + zlds[q]) = mlp_act8<DT>(rz[q], rb[q], zok[q]);
#pragma unroll
      for (int q = 0; q < NW; ++q) *(uint4*)(sb + wlds[q]) = rwv[q];
    };

    f32x4_t acc[NF][PT];
#pragma unroll
    for (int i = 0; i < NF; ++i)
#pragma unroll
      for (int j = 0; j < PT; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};

    gload(0);
    lstore(0);
    __syncthreads();
    for (int s = 0; s < nsteps; ++s) {
      const int cur = s & 1;
      if (s + 1 < nsteps) gload(s + 1);  // in flight behind this step's MFMAs
      const char* sb = smem + cur * STAGE;
#pragma unroll
      for (int kk = 0; kk < BK / 32; ++kk) {
        const int ch = kk * 4 + fq;
        vec8 af[NF], bf[PT];
#pragma unroll
        for (int i = 0; i < NF; ++i) {
          const int row = wn0 + ml_frag_ch(i, fr);
          af[i] = *(const vec8*)(sb + HB + row * ROWB + ((ch ^ ml_swz<BK>(row)) << 4));
        }
#pragma unroll
        for (int j = 0; j < PT; ++j) {
          const int row = j * 16 + fr;
          bf[j] = *(const vec8*)(sb + row * ROWB + ((ch ^ ml_swz<BK>(row)) << 4));
        }
#pragma unroll
        for (int i = 0; i < NF; ++i) {
          if (!gok[i >> 1]) continue;
#pragma unroll
          for (int j = 0; j < PT; ++j) acc[i][j] = E::mfma16x16x32(af[i], bf[j], acc[i][j]);
        }
      }
      if (s + 1 < nsteps) lstore(cur ^ 1);  // the other buffer: last read before the previous barrier
      __syncthreads();
    }

    // fragment pair p gives the lane channels n0 + wn0 + p * 32 + 8 * fq + [0, 8) of row j * 16 + fr
#pragma unroll
    for (int j = 0; j < PT; ++j) {
      const int row = j * 16 + fr;
#pragma unroll
      for (int p = 0; p < NGW; ++p) {
        if (!gok[p]) continue;
        const int ch = n0 + wn0 + p * 32 + 8 * fq;
        uint4 pk;
        pk.x = E::pack2(acc[2 * p][j][0] + bo[p][0], acc[2 * p][j][1] + bo[p][1]);
        pk.y = E::pack2(acc[2 * p][j][2] + bo[p][2], acc[2 * p][j][3] + bo[p][3]);
        pk.z = E::pack2(acc[2 * p + 1][j][0] + bo[p][4], acc[2 * p + 1][j][1] + bo[p][5]);
        pk.w = E::pack2(acc[2 * p + 1][j][2] + bo[p][6], acc[2 * p + 1][j][3] + bo[p][7]);
        const uint32_t off = (row < rows && ch < Co) ? ((uint32_t)row * (uint32_t)Co + (uint32_t)ch) * 2u : kOOB;
        ml_store16(ro, off, pk);
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------ backward data
// out channels n = hidden channels (N = Hd), reduction R = Co.  A block owns a slice of 128 hidden channels
// (blockIdx.x % nslices) and walks 128-row tiles; srows[blockIdx.x / nslices][Hd] takes its column sums.
template <int DT>
__global__ __launch_bounds__(256) void mlp_fc2_dgrad_kernel(const uint16_t* __restrict__ dy,
                                                            const uint16_t* __restrict__ w2t,
                                                            const uint16_t* __restrict__ z0,
                                                            const float* __restrict__ b1, uint16_t* __restrict__ dz,
                                                            int64_t M, int Hd, int Co, int nslices, int mtiles,
                                                            float* __restrict__ srows) {
  using E = E16<DT>;
  typedef typename E::vec8 vec8;
  constexpr int NG = 4, PT = 2;
  constexpr int NF = NG * 2, WR = PT * 16, BR = 4 * WR;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int fr = lane & 15, fq = lane >> 4;
  const int slice = blockIdx.x % nslices;
  const int n0 = slice * (NG * 32);
  const int tstride = gridDim.x / nslices;
  const int N = Hd, R = Co;
  const __amdgpu_buffer_rsrc_t rb = make_rsrc(w2t, (uint32_t)N * (uint32_t)R * 2u);  // <= 2 MiB

  bool gok[NG];
#pragma unroll
  for (int p = 0; p < NG; ++p) gok[p] = n0 + p * 32 < N;
  uint32_t wrow[NF];
#pragma unroll
  for (int i = 0; i < NF; ++i) {
    const int ch = n0 + ml_frag_ch(i, fr);
    wrow[i] = ch < N ? (uint32_t)ch * (uint32_t)R * 2u : kOOB;
  }
  auto kpart = [&](int kk) {
    const int k = kk * 32 + fq * 8;
    return k < R ? (uint32_t)k * 2u : kOOB;
  };
  const int ksteps = (R + 31) >> 5;

  float bh[NG][8];  // b1 of the lane's 8 hidden channels per group
  float st[NG][8];  // their column sums over every tile of the block
#pragma unroll
  for (int p = 0; p < NG; ++p) {
    ml_bias8(b1, n0 + p * 32 + 8 * fq, N, bh[p]);
#pragma unroll
    for (int e = 0; e < 8; ++e) st[p][e] = 0.f;
  }

  for (int t = blockIdx.x / nslices; t < mtiles; t += tstride) {
    const int64_t m0 = (int64_t)t * BR;
    const int64_t left = M - m0;
    const int rows = left < BR ? (int)left : BR;
    const __amdgpu_buffer_rsrc_t ri = make_rsrc(dy + m0 * R, (uint32_t)rows * (uint32_t)R * 2u);
    const __amdgpu_buffer_rsrc_t rz = make_rsrc(z0 + m0 * N, (uint32_t)rows * (uint32_t)N * 2u);
    const __amdgpu_buffer_rsrc_t ro = make_rsrc(dz + m0 * N, (uint32_t)rows * (uint32_t)N * 2u);
    uint32_t xrow[PT];
#pragma unroll
    for (int j = 0; j < PT; ++j) {
      const int row = wave * WR + j * 16 + fr;
      xrow[j] = row < rows ? (uint32_t)row * (uint32_t)R * 2u : kOOB;
    }

    f32x4_t acc[NF][PT];
#pragma unroll
    for (int i = 0; i < NF; ++i)
#pragma unroll
      for (int j = 0; j < PT; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};

    vec8 a0[NF], b0[PT];
    auto load_step = [&](int kk, vec8(&a)[NF], vec8(&b)[PT]) {
      const uint32_t kb = kpart(kk);  // past the reduction: every chunk is kOOB (zeros, no memory traffic)
#pragma unroll
      for (int i = 0; i < NF; ++i)
        a[i] = __builtin_bit_cast(vec8, ml_load16(rb, gok[i >> 1] ? ml_off(wrow[i], kb) : kOOB));
#pragma unroll
      for (int j = 0; j < PT; ++j) b[j] = __builtin_bit_cast(vec8, ml_load16(ri, ml_off(xrow[j], kb)));
    };
    load_step(0, a0, b0);
    for (int kk = 0; kk < ksteps; ++kk) {
      vec8 a1[NF], b1f[PT];
      load_step(kk + 1, a1, b1f);
#pragma unroll
      for (int i = 0; i < NF; ++i) {
        if (!gok[i >> 1]) continue;
#pragma unroll
        for (int j = 0; j < PT; ++j) acc[i][j] = E::mfma16x16x32(a0[i], b0[j], acc[i][j]);
      }
#pragma unroll
      for (int i = 0; i < NF; ++i) a0[i] = a1[i];
#pragma unroll
      for (int j = 0; j < PT; ++j) b0[j] = b1f[j];
    }

    // the lane's 16 bytes of z0 per (row fragment, group): the offsets of its stores
    uint32_t eoff[PT][NG];
    uint4 zv[PT][NG];
#pragma unroll
    for (int j = 0; j < PT; ++j) {
      const int row = wave * WR + j * 16 + fr;
#pragma unroll
      for (int p = 0; p < NG; ++p) {
        const int ch = n0 + p * 32 + 8 * fq;
        eoff[j][p] = (gok[p] && row < rows && ch < N) ? ((uint32_t)row * (uint32_t)N + (uint32_t)ch) * 2u : kOOB;
        zv[j][p] = ml_load16(rz, eoff[j][p]);
      }
    }
#pragma unroll
    for (int j = 0; j < PT; ++j) {
#pragma unroll
      for (int p = 0; p < NG; ++p) {
        if (!gok[p]) continue;
        uint16_t ze[8];
        unpack8(zv[j][p], ze);
        float d[8];
#pragma unroll
        for (int e = 0; e < 8; ++e)
          d[e] = acc[2 * p + (e >> 2)][j][e & 3] * mlp_gelu_grad(E::to_f(ze[e]) + bh[p][e]);
        uint4 pk;
        pk.x = E::pack2(d[0], d[1]);
        pk.y = E::pack2(d[2], d[3]);
        pk.z = E::pack2(d[4], d[5]);
        pk.w = E::pack2(d[6], d[7]);
        ml_store16(ro, eoff[j][p], pk);
        // rows past M and channels past Hd come from zero-filled operands: exactly 0, they add nothing
        uint16_t h[8];
        unpack8(pk, h);
#pragma unroll
        for (int e = 0; e < 8; ++e) st[p][e] += E::to_f(h[e]);
      }
    }
  }

  __shared__ float red[4][NG * 32];
#pragma unroll
  for (int p = 0; p < NG; ++p)
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float t = ml_row16_fold(st[p][e]);
      if (fr == 0) red[wave][p * 32 + 8 * fq + e] = t;
    }
  __syncthreads();
  const int idx = threadIdx.x;
  if (idx < NG * 32 && n0 + idx < N) {
    float t = red[0][idx];
#pragma unroll
    for (int w = 1; w < 4; ++w) t += red[w][idx];
    srows[(int64_t)(blockIdx.x / nslices) * N + n0 + idx] = t;
  }
}

// ------------------------------------------------------------------------------------------------ weight gradient
// chunk swizzle of a [row][64 ch] (128-byte row) LDS image read by ds_read_b64_tr_b16 (conv_wgrad.hip's)
PDT_DEVICE int ml_tr_swz(int row) { return (((row >> 1) & 1) << 1) | (((row >> 3) & 1) << 2); }

// dw2[Co][Hd] tile (64 hidden c x 64 output k) of one split of the rows: pwconv_wgrad_kernel with x = h, made from
// the z0 chunks in registers when they are written to the LDS image
template <int DT>
__global__ __launch_bounds__(256) void mlp_fc2_wgrad_kernel(const uint16_t* __restrict__ z0,
                                                            const float* __restrict__ b1,
                                                            const uint16_t* __restrict__ dy, float* __restrict__ ws,
                                                            int M, int Hd, int Co, int rps, int h_tiles, int o_tiles) {
  using E = E16<DT>;
  typedef typename E::vec8 vec8;
  constexpr int BKP = 128;        // rows per reduction step
  constexpr int ROWB = 128;       // 64 channels * 2 B
  constexpr int XB = BKP * ROWB;  // bytes of one operand's tile
  constexpr int STAGE = 2 * XB;
  __shared__ __attribute__((aligned(1024))) char smem[2 * STAGE];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  // consecutive blocks = the tiles of ONE row range: its rows come from HBM once and from L2 after that
  const int ntile = h_tiles * o_tiles;
  const int tile = blockIdx.x % ntile, split = blockIdx.x / ntile;
  const int kt = tile % o_tiles, ct = tile / o_tiles;
  const int c0 = ct * 64, k0 = kt * 64;
  const int row_begin = split * rps;
  const int row_end = min(M, row_begin + rps);
  const int nsteps = (row_end - row_begin + BKP - 1) / BKP;

  // staging geometry: piece (wave * 4 + j) is 8 rows x 8 chunks = 1 KiB, LDS chunk pch of a row holds the source
  // chunk pch ^ swz(row); swz(row) depends on bit 1 of lrow and on j & 1 only, so a thread meets two hidden chunks
  const int lrow = lane >> 3, pch = lane & 7;
  float bb[2][8];
#pragma unroll
  for (int jp = 0; jp < 2; ++jp) ml_bias8(b1, c0 + (pch ^ ml_tr_swz(jp * 8 + lrow)) * 8, Hd, bb[jp]);

  uint4 rx[4], ry[4];
  bool okx[4];
  auto gload = [&](int step) {
    const int pb = row_begin + step * BKP;
    const int rows = min(BKP, row_end - pb);
    const __amdgpu_buffer_rsrc_t rsx = make_rsrc(z0 + (int64_t)pb * Hd, (uint32_t)(rows * Hd * 2));
    const __amdgpu_buffer_rsrc_t rsy = make_rsrc(dy + (int64_t)pb * Co, (uint32_t)(rows * Co * 2));
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int row = (wave * 4 + j) * 8 + lrow;
      const int lch = pch ^ ml_tr_swz(row);
      const int c = c0 + lch * 8, k = k0 + lch * 8;
      okx[j] = row < rows && c < Hd;
      rx[j] = ml_load16(rsx, okx[j] ? (uint32_t)((row * Hd + c) * 2) : kOOB);
      ry[j] = ml_load16(rsy, (row < rows && k < Co) ? (uint32_t)((row * Co + k) * 2) : kOOB);
    }
  };
  auto lstore = [&](int buf) {
    char* sb = smem + buf * STAGE + (wave * 4) * 1024 + lane * 16;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      *(uint4*)(sb + j * 1024) = mlp_act8<DT>(rx[j], bb[j & 1], okx[j]);
      *(uint4*)(sb + XB + j * 1024) = ry[j];
    }
  };

  f32x4_t acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  // transposed-read lane geometry: group g = lane >> 4 holds rows 8g .. 8g + 7 of the wave's 32-row slice
  const int g = lane >> 4, li = lane & 15, q = li >> 2, p4 = li & 3;

  if (nsteps > 0) {  // block-uniform
    gload(0);
    lstore(0);
    __syncthreads();
    for (int s = 0; s < nsteps; ++s) {
      const int cur = s & 1;
      if (s + 1 < nsteps) gload(s + 1);  // in flight behind this step's MFMAs
      const char* sb = smem + cur * STAGE;
      vec8 af[4], bfr[4];
#pragma unroll
      for (int f = 0; f < 4; ++f) {
        const int r0 = wave * 32 + 8 * g + q, r1 = r0 + 4;
        const int col = f * 16 + 4 * p4;  // element within the 64-wide row
        const int ch = col >> 3, off = (col & 7) * 2;
        const int o0 = r0 * ROWB + ((ch ^ ml_tr_swz(r0)) << 4) + off;
        const int o1 = r1 * ROWB + ((ch ^ ml_tr_swz(r1)) << 4) + off;
        s16x4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((ml_lds_s16x4*)(sb + o0));
        s16x4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((ml_lds_s16x4*)(sb + o1));
        af[f] = __builtin_bit_cast(vec8, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
        lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((ml_lds_s16x4*)(sb + XB + o0));
        hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((ml_lds_s16x4*)(sb + XB + o1));
        bfr[f] = __builtin_bit_cast(vec8, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
      }
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = E::mfma16x16x32(af[i], bfr[j], acc[i][j]);
      if (s + 1 < nsteps) lstore(cur ^ 1);  // the other buffer: last read before the previous barrier
      __syncthreads();
    }
  }

  // sum the 4 waves' tiles through LDS in wave order; acc[i][j]: rows c = 16i + 4 * (lane >> 4) + r, col k = 16j + (lane & 15)
  float* red = (float*)smem;  // [4 waves][64 k][64 c]
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int k = 16 * j + (lane & 15);
      const int c = 16 * i + 4 * (lane >> 4);
      *(f32x4_t*)(red + (wave * 64 + k) * 64 + c) = acc[i][j];
    }
  __syncthreads();
  float* slab = ws + (int64_t)split * Co * Hd;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int idx = (e * 256 + tid) * 4;  // 0 .. 4095
    const int k = idx >> 6, c = idx & 63;
    f32x4_t v = *(f32x4_t*)(red + k * 64 + c);
#pragma unroll
    for (int w = 1; w < 4; ++w) v += *(f32x4_t*)(red + (w * 64 + k) * 64 + c);
    // Hd % 8 == 0: a group of 4 channels is wholly in or out
    if (k0 + k < Co && c0 + c < Hd) *(f32x4_t*)(slab + (int64_t)(k0 + k) * Hd + c0 + c) = v;
  }
}

// persistent blocks the GEMMs aim for: a few per CU (256 CUs)
constexpr int kMlpGemmBlocks = 1536;

void mlp_check(const char* op, int64_t M, int Hd, int Co) {
  if (!mlp_fits(M, 8, Hd, Co)) pdt_hip_fail(op, hipErrorInvalidValue, __FILE__, __LINE__);
}

template <int DT, int NGW, int BK>
void mlp_fwd_go(const uint16_t* z0, const float* b1, const uint16_t* w2, const float* b2, uint16_t* y, int64_t M, int Hd,
                int Co, hipStream_t s) {
  constexpr int NB = 4 * NGW * 32;
  const int ncb = (Co + NB - 1) / NB;
  const int mtiles = (int)((M + 63) / 64);
  int per = kMlpGemmBlocks / ncb;
  if (per > mtiles) per = mtiles;
  hipLaunchKernelGGL((mlp_fc2_fwd_kernel<DT, NGW, BK>), dim3((unsigned)(per * ncb)), dim3(256), 0, s, z0, b1, w2, b2, y,
                     M, Hd, Co, ncb, mtiles);
}

template <int DT>
void mlp_fwd_dt(const uint16_t* z0, const float* b1, const uint16_t* w2, const float* b2, uint16_t* y, int64_t M, int Hd,
                int Co, hipStream_t s) {
  // the column block follows the output width alone: 128 channels with 64-wide steps, or 256 with 32-wide ones
  if (Co <= 128) mlp_fwd_go<DT, 1, 64>(z0, b1, w2, b2, y, M, Hd, Co, s);
  else mlp_fwd_go<DT, 2, 32>(z0, b1, w2, b2, y, M, Hd, Co, s);
}

}  // namespace

void mlp_fc2_fwd_launch(int dtype, const uint16_t* z0, const float* b1, const uint16_t* w2, const float* b2,
                        uint16_t* y, int64_t M, int Hd, int Co, hipStream_t s) {
  mlp_check("mlp_fc2_fwd_launch: operand outside the kernels' contract", M, Hd, Co);
  PDT_COUNT("mlp_fc2_fwd");
  if (dtype == kBF16) mlp_fwd_dt<kBF16>(z0, b1, w2, b2, y, M, Hd, Co, s);
  else mlp_fwd_dt<kF16>(z0, b1, w2, b2, y, M, Hd, Co, s);
}

MlpDgradPlan mlp_fc2_dgrad_launch(int dtype, const uint16_t* dy, const uint16_t* w2t, const uint16_t* z0,
                                  const float* b1, uint16_t* dz, float* db1, int64_t M, int Hd, int Co, int max_blocks,
                                  hipStream_t s) {
  mlp_check("mlp_fc2_dgrad_launch: operand outside the kernels' contract", M, Hd, Co);
  if (max_blocks < 0) pdt_hip_fail("mlp_fc2_dgrad_launch: bad max_blocks", hipErrorInvalidValue, __FILE__, __LINE__);
  PDT_COUNT("mlp_fc2_dgrad");
  if (max_blocks == 0) max_blocks = kMlpGemmBlocks;
  const int nslices = (Hd + 127) / 128;
  const int mtiles = (int)((M + 127) / 128);
  int per = max_blocks / nslices;
  if (per < 1) per = 1;
  if (per > mtiles) per = mtiles;
  const dim3 g((unsigned)(per * nslices));
  // every block owns at least one tile (per <= mtiles) and writes its slice of its partial row exactly once
  Scratch part((size_t)per * Hd * sizeof(float), s);
  float* srows = part.as<float>();
  if (dtype == kBF16)
    hipLaunchKernelGGL((mlp_fc2_dgrad_kernel<kBF16>), g, dim3(256), 0, s, dy, w2t, z0, b1, dz, M, Hd, Co, nslices,
                       mtiles, srows);
  else
    hipLaunchKernelGGL((mlp_fc2_dgrad_kernel<kF16>), g, dim3(256), 0, s, dy, w2t, z0, b1, dz, M, Hd, Co, nslices, mtiles,
                       srows);
  wgrad_reduce_launch(srows, per, 1, Hd, Hd, Hd, db1, Hd, 1.f, false, s);
  // the lane's chain over its tiles (2 rows each), the 16-lane fold, the 4-wave fold, the partial rows
  return MlpDgradPlan{per, (mtiles + per - 1) / per * 2 + 4 + 4 + per};
}

MlpWgradPlan mlp_fc2_wgrad_plan(int64_t M, int Hd, int Co, int target_blocks) {
  MlpWgradPlan pl{};
  pl.h_tiles = (Hd + 63) / 64;
  pl.o_tiles = (Co + 63) / 64;
  const int64_t tiles = (int64_t)pl.h_tiles * pl.o_tiles;
  int64_t splits = ((int64_t)target_blocks + tiles - 1) / tiles;
  const int64_t most = (M + 127) / 128;  // at least one reduction step per split
  if (splits > most) splits = most;
  if (splits > 4096) splits = 4096;  // bounds the slab workspace
  if (splits < 1) splits = 1;
  int64_t rps = M > 0 ? (M + splits - 1) / splits : 128;
  rps = (rps + 127) / 128 * 128;
  pl.rows_per_split = (int)rps;
  pl.splits = M > 0 ? (int)((M + rps - 1) / rps) : 1;
  // every product of a split's rows, the 4-wave fold and the slabs, each accumulation worth one fp32 ulp (2 * 2^-24)
  const int64_t chain = 2 * (rps + 4 + pl.splits);
  pl.chain = (int)(chain < INT32_MAX ? chain : INT32_MAX);
  return pl;
}

void mlp_fc2_wgrad_launch(int dtype, const uint16_t* z0, const float* b1, const uint16_t* dy, float* ws, int64_t M,
                          int Hd, int Co, const MlpWgradPlan& plan, hipStream_t s) {
  mlp_check("mlp_fc2_wgrad_launch: operand outside the kernels' contract", M, Hd, Co);
  PDT_COUNT("mlp_fc2_wgrad");
  const dim3 g((unsigned)(plan.h_tiles * plan.o_tiles * plan.splits));
  if (dtype == kBF16)
    hipLaunchKernelGGL((mlp_fc2_wgrad_kernel<kBF16>), g, dim3(256), 0, s, z0, b1, dy, ws, (int)M, Hd, Co,
                       plan.rows_per_split, plan.h_tiles, plan.o_tiles);
  else
    hipLaunchKernelGGL((mlp_fc2_wgrad_kernel<kF16>), g, dim3(256), 0, s, z0, b1, dy, ws, (int)M, Hd, Co,
                       plan.rows_per_split, plan.h_tiles, plan.o_tiles);
}

}  // namespace pdt
