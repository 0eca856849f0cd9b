#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "col_reduce.h"

namespace pdt {
// activation fused behind the BatchNorm (torch's breakpoint conventions, see bnact.hip)
enum BnAct : int { kActIdentity = 0, kActRelu = 1, kActRelu6 = 2, kActHardswish = 3 };

constexpr int kBnActMaxC = 2048;

// How a [rows, C] tensor is spread over 256-thread blocks: a block owns `cvb` consecutive 8-channel groups
// (`chunks` such column chunks cover a row) and `rpi` row lanes; the two reduce kernels run `blocks` row blocks.
// col_plan (col_reduce.h) with the cvb that idles the fewest lanes.
using BnActPlan = ColPlan;
BnActPlan bnact_plan(int64_t rows, int C);

void bnact_stats_launch(int dtype, const uint16_t* x, double* slots, int64_t rows, int C, const BnActPlan& p,
                        hipStream_t s);
void bnact_fwd_launch(int dtype, int act, const uint16_t* x, const float* coef, uint16_t* out, int64_t rows, int C,
                      const BnActPlan& p, hipStream_t s);
void bnact_bwd_reduce_launch(int dtype, int act, const uint16_t* g, const uint16_t* x, const float* coef, double* slots,
                             int64_t rows, int C, const BnActPlan& p, hipStream_t s);
void bnact_bwd_apply_launch(int dtype, int act, const uint16_t* g, const uint16_t* x, const float* coef,
                            const float* bcoef, uint16_t* dx, int64_t rows, int C, const BnActPlan& p, hipStream_t s);
}  // namespace pdt
