// kfn_loss_scale.hip -- dynamic loss scaling for mixed-precision training (gfx950): scale the loss gradient, unscale and
// check the weight gradients, and TensorFlow's Adam guarded by the overflow flag, all driven by one small state record in
// device memory (kfn_loss_scale_state), so that a step needs no read-back.  DESIGN.md 6h.
#include "kfn_common.h"

namespace {

constexpr float MAX_SCALE = 16777216.0f;   // 2^24

__global__ __launch_bounds__(256) void scale_kernel(float* __restrict__ buf, long n, const kfn_loss_scale_state* __restrict__ st) {
  const float s = st->scale;   // a power of two: the products are exact unless they leave fp32's range
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) buf[i] *= s;
}

__global__ __launch_bounds__(256) void unscale_check_kernel(float* __restrict__ g, long n, kfn_loss_scale_state* st) {
  const float inv = 1.0f / st->scale;
  int bad = 0;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const float v = g[i];
    bad |= !(fabsf(v) <= 3.402823466e+38f);   // inf or NaN
    g[i] = v * inv;
  }
  if (bad) atomicOr(&st->overflow, 1);   // an integer OR: the order does not matter
}

// adam_step_kernel (kfn_train_loss.hip) behind the flag, with the bias correction from the state's accumulators
__global__ __launch_bounds__(256) void adam_guarded_kernel(float* __restrict__ w, float* __restrict__ m, float* __restrict__ v,
                                                           const float* __restrict__ g, long n, double lr, double b1, double b2,
                                                           double eps, double wd, const kfn_loss_scale_state* __restrict__ st) {
  if (st->overflow != 0) return;
  const double p1 = st->beta1_power * b1, p2 = st->beta2_power * b2;   // beta^t of THIS update
  const double lr_t = lr * sqrt(1.0 - p2) / (1.0 - p1);
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const double wi = (double)w[i];
    const double gi = (double)g[i] + wd * wi;
    const float mf = (float)(b1 * (double)m[i] + (1.0 - b1) * gi);
    const float vf = (float)(b2 * (double)v[i] + (1.0 - b2) * (gi * gi));
    m[i] = mf;
    v[i] = vf;
    w[i] = (float)(wi - lr_t * (double)mf / (sqrt((double)vf) + eps));
  }
}

// one thread, after every thread of adam_guarded_kernel has read the state (a later launch on the same stream)
__global__ void loss_scale_update_kernel(kfn_loss_scale_state* st, double b1, double b2, int growth_interval) {
  if (st->overflow != 0) {
    const float half = st->scale * 0.5f;
    st->scale = half < 1.0f ? 1.0f : half;
    st->good_steps = 0;
    st->skipped += 1;
    st->overflow = 0;
  } else {
    st->beta1_power *= b1;
    st->beta2_power *= b2;
    st->adam_t += 1;
    st->good_steps += 1;
    if (st->good_steps >= growth_interval) {
      const float twice = st->scale * 2.0f;
      st->scale = twice > MAX_SCALE ? MAX_SCALE : twice;
      st->good_steps = 0;
    }
  }
}

unsigned blocks_for(long n) {
  long b = (n + 255) / 256;
  return (unsigned)(b < 1 ? 1 : (b > 16384 ? 16384 : b));
}

}  // namespace

extern "C" int kfn_loss_scale_apply(float* buf, long n, const kfn_loss_scale_state* state, void* stream) {
  KFN_REQUIRE(buf && state && n > 0, "kfn_loss_scale_apply: null argument or n = %ld", n);
  hipLaunchKernelGGL(scale_kernel, dim3(blocks_for(n)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), buf, n, state);
  KFN_LAUNCH_CHECK("scale_kernel");
  return KFN_OK;
}

extern "C" int kfn_loss_scale_unscale_check(float* grads, long n, kfn_loss_scale_state* state, void* stream) {
  KFN_REQUIRE(grads && state && n > 0, "kfn_loss_scale_unscale_check: null argument or n = %ld", n);
  hipLaunchKernelGGL(unscale_check_kernel, dim3(blocks_for(n)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), grads, n, state);
  KFN_LAUNCH_CHECK("unscale_check_kernel");
  return KFN_OK;
}

extern "C" int kfn_adam_step_guarded(float* w, float* m, float* v, const float* g, long n, double lr, double beta1, double beta2,
                                     double epsilon, double weight_decay, int growth_interval, kfn_loss_scale_state* state,
                                     void* stream) {
  KFN_REQUIRE(w && m && v && g && state, "kfn_adam_step_guarded: null argument");
  KFN_REQUIRE(n > 0, "kfn_adam_step_guarded: n = %ld", n);
  KFN_REQUIRE(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0 && epsilon > 0.0 && weight_decay >= 0.0 && lr == lr,
              "kfn_adam_step_guarded: bad hyper-parameters");
  KFN_REQUIRE(growth_interval >= 1, "kfn_adam_step_guarded: growth_interval = %d", growth_interval);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(adam_guarded_kernel, dim3(blocks_for(n)), dim3(256), 0, s, w, m, v, g, n, lr, beta1, beta2, epsilon,
                     weight_decay, state);
  KFN_LAUNCH_CHECK("adam_guarded_kernel");
  hipLaunchKernelGGL(loss_scale_update_kernel, dim3(1), dim3(1), 0, s, state, beta1, beta2, growth_interval);
  KFN_LAUNCH_CHECK("loss_scale_update_kernel");
  return KFN_OK;
}
