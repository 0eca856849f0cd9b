#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
// Squeeze-and-excitation kernels (se.hip): y = x * gate(W2 act(W1 mean_hw(x) + b1) + b2) over a dense NHWC tensor
// x[N][HW][C], 16-bit, C % 8 == 0, 8 <= C <= 4096, 1 <= S <= 512, N * HW * C < 2^40, 16-byte aligned.  W1[S][C],
// b1[S], W2[C][S], b2[C] and everything per image (z[N][C], u[N][S], s[N][C], dv[N][C], du[N][S], g[N][C]) are fp32;
// y and dx have the dtype of x and are rounded once.  No atomics: every sum has an order fixed by the shape and the plan.
namespace pdt {
enum SeAct { kSeRelu = 0, kSeSilu = 1 };
enum SeGate { kSeSigmoid = 0, kSeHardsigmoid = 1 };

struct SePlan {
  int chunks;              // blocks that share the HW rows of one image (= partial rows per image)
  int64_t rows_per_chunk;  // rows of a chunk; chunks * rows_per_chunk >= HW, the last chunk may be short
};
bool se_fits(int64_t N, int64_t HW, int64_t C, int64_t S);
// chunks from HW, the row lanes of a block and what `max_blocks` leaves per image (N * chunks <= max_blocks whenever
// N <= max_blocks); it fixes the summation order of the two reductions
SePlan se_plan(int64_t N, int64_t HW, int C, int max_blocks);

// partial[N][chunks][C] = per-chunk sums of x over its rows
void se_pool_launch(int dtype, const uint16_t* x, float* partial, int64_t N, int64_t HW, int C, const SePlan& plan,
                    hipStream_t s);
// z = fold(partial) / HW, u = W1 z + b1, sg = gate(W2 act(u) + b2)
void se_gate_launch(int act, int gate, const float* partial, const float* w1, const float* b1, const float* w2,
                    const float* b2, float* z, float* u, float* sg, int64_t N, int64_t HW, int C, int S, int chunks,
                    hipStream_t s);
// y = round(x * sg), persistent blocks (at most max_blocks per column chunk)
void se_scale_launch(int dtype, const uint16_t* x, const float* sg, uint16_t* y, int64_t N, int64_t HW, int C,
                     int max_blocks, hipStream_t s);
// partial[N][chunks][C] = per-chunk sums of dy * x
void se_bwd_reduce_launch(int dtype, const uint16_t* dy, const uint16_t* x, float* partial, int64_t N, int64_t HW, int C,
                          const SePlan& plan, hipStream_t s);
// dv = fold(partial) * gate'(sg), du = (W2^T dv) * act'(u), g = (W1^T du) / HW
void se_gate_bwd_launch(int act, int gate, const float* partial, const float* w1, const float* w2, const float* u,
                        const float* sg, float* dv, float* du, float* g, int64_t N, int64_t HW, int C, int S, int chunks,
                        hipStream_t s);
// dW2 = sum_n dv act(u)^T, db2 = sum_n dv, dW1 = sum_n du z^T, db1 = sum_n du: one thread per element, images in order
void se_wgrad_launch(int act, const float* dv, const float* du, const float* z, const float* u, float* dw1, float* db1,
                     float* dw2, float* db2, int64_t N, int C, int S, hipStream_t s);
// dx = round(dy * sg + g)
void se_bwd_apply_launch(int dtype, const uint16_t* dy, const float* sg, const float* g, uint16_t* dx, int64_t N,
                         int64_t HW, int C, int max_blocks, hipStream_t s);
}  // namespace pdt
