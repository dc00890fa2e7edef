// kfn_train_shared.h -- what the weight-gradient launches of kfn_train.hip (fp32 operands) and kfn_train_f16.hip (fp16
// operands) have in common: the kernel arguments and the plan that cuts the pixels into runs.
#pragma once
#include "kfn_common.h"

namespace kfn {

constexpr int WG_BM = 128;         // k rows per workgroup
constexpr int WG_BP = 16;          // pixels per stage, fp32 operands
constexpr int WG_BP_F16 = 32;      // pixels per stage, fp16 operands (two k-steps of v_mfma_f32_32x32x16_f16)

struct WgradArgs {
  const float* x;
  const float* dz;
  float* ws;
  int H, W, Cin, ldx, Cout, ldz, kw, stride, Ho, Wo, pad_t, pad_l;
  int Ktot;       // kh*kw*Cin; row Ktot is the bias row
  long P;         // N*Ho*Wo
  long chunk;     // pixels per split (multiple of the stage)
  int tiles_n;
  int vec_b;      // dZ rows can be read as float4 (ldz % 4 == 0, 16-byte aligned base)
};

struct WgradPlan {
  int Ho, Wo, pad_t, pad_l, Ktot, tn, tiles_m, tiles_n, splits;
  long P, chunk;
};

// kfn_train_f16.hip: the fp16-operand GEMM into the workspace planes (the caller reduces them as for fp32)
int wgrad_f16_launch(const WgradArgs& a, const WgradPlan& pl, hipStream_t s);

}  // namespace kfn
