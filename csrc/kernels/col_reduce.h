// Deterministic per-channel column sums over a [rows, C] tensor: the one scheme behind every BatchNorm statistic and
// backward sum that is not a conv epilogue (bn.hip, pool.hip, fp32.hip, bnact.hip).
//
// A thread owns ONE fixed group of G consecutive channels (8 for 16-bit, 4 for fp32) and walks rows in fp32 chains.
// A 256-thread block is cvb channel groups x rpi row lanes; a row of C / G groups is split into `chunks` column chunks
// of cvb groups (grid.y; one chunk of C / G groups for every kernel but bnact's).  The row lanes are summed in LDS in a
// fixed order, the block writes one partial row [C][K] of srows, and stat_rows_reduce folds the partial rows into the
// kStatSlots fp64 slots (conv_fwd.h).  No atomics anywhere: seeded runs repeat bit for bit.
// Only the per-row body (loads, mask, xhat, accumulation) belongs to a kernel.
#pragma once
#include "../common.h"
#include "conv_fwd.h"

namespace pdt {

// cvb groups x rpi row lanes per block, `chunks` column chunks (grid.y), `blocks` row blocks (grid.x), lds bytes of
// the [rpi][cvb * G][K] float staging array.
struct ColPlan {
  int cvb, rpi, chunks, blocks;
  size_t lds;
};

// blocks: at least rows_per_thread rows per thread, at most block_cap row blocks.  cvb = 0: one chunk of all C / G
// groups (the kernels without column chunks, which therefore stop at 256 groups).
inline ColPlan col_plan(int64_t rows, int C, int G, int K, int rows_per_thread, int block_cap, int cvb = 0) {
  if (C <= 0 || C % G != 0)
    pdt_hip_fail("col_reduce: C must be a positive multiple of the group width", hipErrorInvalidValue, __FILE__,
                 __LINE__);
  const int groups = C / G;
  if (cvb == 0) cvb = groups;
  if (cvb < 1 || cvb > 256)
    pdt_hip_fail("col_reduce: more than 256 channel groups in one chunk", hipErrorInvalidValue, __FILE__, __LINE__);
  const int rpi = 256 / cvb;
  const int64_t per = (int64_t)rpi * rows_per_thread;
  int64_t b = (rows + per - 1) / per;
  if (b > block_cap) b = block_cap;
  return ColPlan{cvb, rpi, (groups + cvb - 1) / cvb, (int)(b < 1 ? 1 : b), (size_t)rpi * cvb * G * K * sizeof(float)};
}

// The `blocks` partial rows [C][K] of one reduce: launch(srows) fills them, stat_rows_reduce folds them into slots.
template <typename Launch>
void col_reduce_run(int blocks, int C, int K, double* slots, hipStream_t s, Launch&& launch) {
  Scratch part((size_t)blocks * C * K * sizeof(float), s);
  float* srows = part.as<float>();
  launch(srows);
  stat_rows_reduce_launch(srows, blocks, C * K, slots, s);
}

#ifdef __HIPCC__
// c0: the thread's first channel; rl: its row lane (rows blockIdx.x * rpi + rl, then every gridDim.x * rpi);
// active: it owns data (lanes past rpi * cvb and groups past C idle)
struct ColLane {
  int c0, rl;
  bool active;
};
template <int G>
PDT_DEVICE ColLane col_lanes(int C, int cvb, int rpi) {
  const int cl = threadIdx.x % cvb, rl = threadIdx.x / cvb;
  const int cv = blockIdx.y * cvb + cl;
  return ColLane{cv * G, rl, rl < rpi && cv * G < C};
}

// one group's accumulators into red[...][group][G][K]
template <int K, int G>
PDT_DEVICE void col_store(const float (&s)[K][G], float* __restrict__ red, int group) {
#pragma unroll
  for (int e = 0; e < G; ++e)
#pragma unroll
    for (int k = 0; k < K; ++k) red[(group * G + e) * K + k] = s[k][e];
}

// the fixed-order sum over the row lanes: `per` = entries of this chunk's part of the block's partial row
template <int K>
PDT_DEVICE void col_rows_sum(const float* __restrict__ red, float* __restrict__ srows, int C, int per, int rpi) {
  __syncthreads();
  const int col0 = blockIdx.y * per;  // its first column of the [C * K] row
  float* dst = srows + (int64_t)blockIdx.x * C * K;
  for (int idx = threadIdx.x; idx < per && col0 + idx < C * K; idx += 256) {
    float t = 0.f;
    for (int r = 0; r < rpi; ++r) t += red[r * per + idx];
    dst[col0 + idx] = t;
  }
}

// Block reduction over the row lanes and the block's partial row.  red: [rpi][cvb * G][K] floats.
template <int K, int G>
PDT_DEVICE void block_rows_out(const float (&s)[K][G], const ColLane& ln, float* __restrict__ red,
                               float* __restrict__ srows, int C, int cvb, int rpi) {
  if (ln.active) col_store<K, G>(s, red, ln.rl * cvb + threadIdx.x % cvb);
  col_rows_sum<K>(red, srows, C, cvb * G * K, rpi);
}

// The same for a thread that owns NV groups of a row, cvb groups apart (cvb threads per row of NV * cvb groups).
template <int K, int G, int NV>
PDT_DEVICE void block_rows_out(const float (&s)[NV][K][G], const ColLane& ln, float* __restrict__ red,
                               float* __restrict__ srows, int C, int cvb, int rpi) {
  if (ln.active) {
#pragma unroll
    for (int q = 0; q < NV; ++q) col_store<K, G>(s[q], red, ln.rl * NV * cvb + q * cvb + threadIdx.x % cvb);
  }
  col_rows_sum<K>(red, srows, C, NV * cvb * G * K, rpi);
}
#endif  // __HIPCC__

}  // namespace pdt
