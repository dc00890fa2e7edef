// kfn_reproj.hip -- the reference's reprojection loss with its gradient (gfx950).
// Compiled with -ffp-contract=off like kfn_train_loss.hip: every per-cell term is a list of rounded fp32 operations.
//   kfn_reproj_loss_grad  KFNet.ReprojectionLoss (KFNet/KFNet.py:405-428) in its masked form, as MeasureCoordLoss (:246-248),
//                         TemporalCoordLoss (:270-272) and KFCoordLoss (:292-294) add it: the squared distance between the
//                         unit ray of the predicted point in the camera frame and the unit ray of the cell's pixel, for one
//                         to three predictions in one launch, and its gradient ADDED to d(loss)/d(prediction).
// `valid` is read from the stats of the NLL launch that ran before, so the gradient needs no pass of its own: one walk over
// the cells gives the sums and the gradients.
#include "kfn_common.h"

namespace {

constexpr int RT = 1024;        // one workgroup, as the NLL launches: a few 10^4 cells per batch
constexpr float FLOOR = 1e-12f; // tf.nn.l2_normalize's epsilon: x * rsqrt(max(sum(x^2), 1e-12))
constexpr float INV_FLOOR = 1e6f;

struct ReprojArgs {
  const float* x[KFN_REPROJ_MAX_OUTPUTS];
  float* dx[KFN_REPROJ_MAX_OUTPUTS];
  float weight[KFN_REPROJ_MAX_OUTPUTS];
  int ld_x[KFN_REPROJ_MAX_OUTPUTS], ld_dx[KFN_REPROJ_MAX_OUTPUTS];
  int vec_x[KFN_REPROJ_MAX_OUTPUTS], vec_dx[KFN_REPROJ_MAX_OUTPUTS];   // 16-byte accesses: ld % 4 == 0, base aligned
  const float* M;
  const float* labels;
  const float* pixel_map;
  const float* valid;
  float* stats;
  int outputs, B, h, w, label_stride;
  float u, v, inv_fx, inv_fy;
};

__device__ __forceinline__ double block_sum(double v, double* red) {
  const int t = threadIdx.x;
  __syncthreads();
  red[t] = v;
  __syncthreads();
  for (int s = RT / 2; s > 0; s >>= 1) {   // a fixed tree: the same sum in every launch
    if (t < s) red[t] += red[t + s];
    __syncthreads();
  }
  return red[0];
}

__global__ __launch_bounds__(RT) void reproj_loss_grad_kernel(ReprojArgs p) {
  __shared__ double red[RT];
  const int t = threadIdx.x;
  const long hw = (long)p.h * p.w, P = (long)p.B * hw;
  const int ls = p.label_stride;
  const long lW = (long)p.w * ls, lH = (long)p.h * ls;
  const float vp1 = *p.valid + 1.0f;      // the reference's valid_pixel + 1, valid_pixel = sum(mask) + 1 (KFNet.py:422, :427)

  double sum[KFN_REPROJ_MAX_OUTPUTS] = {0.0, 0.0, 0.0};
  for (long i = t; i < P; i += RT) {
    const int b = (int)(i / hw);
    const int rem = (int)(i - b * hw);
    const int r = rem / p.w, c = rem % p.w;
    const float mask = p.labels[(((long)b * lH + (long)r * ls) * lW + (long)c * ls) * 4 + 3];
    if (mask != 1.0f) continue;           // m = 0: nothing to add, the gradient buffers keep their bits
    float qx, qy;
    if (p.pixel_map) {
      const float2 pm = reinterpret_cast<const float2*>(p.pixel_map)[rem];
      qx = pm.x; qy = pm.y;
    } else {
      qx = ((float)(8 * c) - p.u) * p.inv_fx;
      qy = ((float)(8 * r) - p.v) * p.inv_fy;
    }
    const float sq = (qx * qx + qy * qy) + 1.0f;
    const float iq = 1.0f / sqrtf(fmaxf(sq, FLOOR));
    const float n0 = qx * iq, n1 = qy * iq, n2 = iq;                   // the pixel's unit ray
    const float4* Mb = reinterpret_cast<const float4*>(p.M + (long)b * 12);
    const float4 m0 = Mb[0], m1 = Mb[1], m2 = Mb[2];                   // rows of M_b = P_b G^-1

    for (int o = 0; o < p.outputs; ++o) {
      const float* xp = p.x[o] + i * p.ld_x[o];
      float x0, x1, x2;
      if (p.vec_x[o]) {
        const float4 xv = *reinterpret_cast<const float4*>(xp);
        x0 = xv.x; x1 = xv.y; x2 = xv.z;
      } else {
        x0 = xp[0]; x1 = xp[1]; x2 = xp[2];
      }
      const float c0 = ((m0.x * x0 + m0.y * x1) + m0.z * x2) + m0.w;
      const float c1 = ((m1.x * x0 + m1.y * x1) + m1.z * x2) + m1.w;
      const float c2 = ((m2.x * x0 + m2.y * x1) + m2.z * x2) + m2.w;
      const float s = (c0 * c0 + c1 * c1) + c2 * c2;
      const bool above = s > FLOOR;
      const float ic = above ? 1.0f / sqrtf(s) : INV_FLOOR;
      const float a0 = c0 * ic, a1 = c1 * ic, a2 = c2 * ic;            // the prediction's unit ray
      const float e0 = a0 - n0, e1 = a1 - n1, e2 = a2 - n2;
      sum[o] += (double)((e0 * e0 + e1 * e1) + e2 * e2);
      float g0, g1, g2;                                                // d(rho)/d(cam)
      if (above) {
        const float dot = (a0 * n0 + a1 * n1) + a2 * n2;
        const float k = 2.0f * ic;
        g0 = k * (a0 * dot - n0); g1 = k * (a1 * dot - n1); g2 = k * (a2 * dot - n2);
      } else {                                                         // the floor: n(cam) = 1e6 cam
        const float k = 2.0f * INV_FLOOR;
        g0 = k * e0; g1 = k * e1; g2 = k * e2;
      }
      const float k = p.weight[o] / vp1;
      const float d0 = k * ((m0.x * g0 + m1.x * g1) + m2.x * g2);      // M_b[:, :3]^T d(rho)/d(cam)
      const float d1 = k * ((m0.y * g0 + m1.y * g1) + m2.y * g2);
      const float d2 = k * ((m0.z * g0 + m1.z * g1) + m2.z * g2);
      float* gp = p.dx[o] + i * p.ld_dx[o];
      if (p.vec_dx[o]) {
        float4 gv = *reinterpret_cast<float4*>(gp);
        gv.x += d0; gv.y += d1; gv.z += d2;                            // .w goes back as it came
        *reinterpret_cast<float4*>(gp) = gv;
      } else {
        gp[0] += d0; gp[1] += d1; gp[2] += d2;
      }
    }
  }
  double R[KFN_REPROJ_MAX_OUTPUTS];
  for (int o = 0; o < KFN_REPROJ_MAX_OUTPUTS; ++o) R[o] = o < p.outputs ? block_sum(sum[o], red) / (double)vp1 : 0.0;
  if (t == 0) {
    double total = 0.0;
    for (int o = 0; o < p.outputs; ++o) total += (double)p.weight[o] * R[o];
    p.stats[0] = (float)R[0]; p.stats[1] = (float)R[1]; p.stats[2] = (float)R[2];
    p.stats[3] = (float)total;
    p.stats[4] = vp1;
    p.stats[5] = p.stats[6] = p.stats[7] = 0.0f;
  }
}

}  // namespace

extern "C" int kfn_reproj_loss_grad(const kfn_reproj_desc* d, const float* M, const float* labels, const float* pixel_map,
                                    const float* nll_stats, int valid_index, float* stats_out, void* stream) {
  KFN_REQUIRE(d && M && labels && nll_stats && stats_out, "kfn_reproj_loss_grad: null argument");
  KFN_REQUIRE(d->struct_size == (int32_t)sizeof(kfn_reproj_desc), "kfn_reproj_loss_grad: struct_size %d, expected %d",
              (int)d->struct_size, (int)sizeof(kfn_reproj_desc));
  KFN_REQUIRE(d->B > 0 && d->h > 0 && d->w > 0 && (long)d->B * d->h * d->w < (1L << 24),
              "kfn_reproj_loss_grad: bad grid %dx%dx%d", d->B, d->h, d->w);
  KFN_REQUIRE(d->label_stride == 1 || d->label_stride == 8, "kfn_reproj_loss_grad: label_stride %d is neither 1 nor 8",
              d->label_stride);
  KFN_REQUIRE(d->outputs >= 1 && d->outputs <= KFN_REPROJ_MAX_OUTPUTS, "kfn_reproj_loss_grad: %d outputs, expected 1..%d",
              d->outputs, KFN_REPROJ_MAX_OUTPUTS);
  KFN_REQUIRE(valid_index >= 0, "kfn_reproj_loss_grad: valid_index %d", valid_index);
  KFN_REQUIRE(((uintptr_t)M & 15) == 0 && ((uintptr_t)labels & 3) == 0 && ((uintptr_t)pixel_map & 7) == 0,
              "kfn_reproj_loss_grad: M must be 16-byte and pixel_map 8-byte aligned");
  ReprojArgs a;
  for (int o = 0; o < KFN_REPROJ_MAX_OUTPUTS; ++o) {
    a.x[o] = nullptr; a.dx[o] = nullptr; a.weight[o] = 0.0f;
    a.ld_x[o] = a.ld_dx[o] = a.vec_x[o] = a.vec_dx[o] = 0;
  }
  for (int o = 0; o < d->outputs; ++o) {
    const kfn_reproj_output& q = d->out[o];
    KFN_REQUIRE(q.x && q.dx, "kfn_reproj_loss_grad: output %d has a null buffer", o);
    KFN_REQUIRE(q.ld_x >= 3 && q.ld_dx >= 3, "kfn_reproj_loss_grad: output %d has pixel strides below 3 (%d, %d)", o, q.ld_x, q.ld_dx);
    KFN_REQUIRE(((uintptr_t)q.x & 3) == 0 && ((uintptr_t)q.dx & 3) == 0, "kfn_reproj_loss_grad: output %d is misaligned", o);
    KFN_REQUIRE(q.weight == q.weight, "kfn_reproj_loss_grad: output %d has a NaN weight", o);
    a.x[o] = q.x; a.dx[o] = q.dx; a.weight[o] = q.weight; a.ld_x[o] = q.ld_x; a.ld_dx[o] = q.ld_dx;
    a.vec_x[o] = q.ld_x % 4 == 0 && ((uintptr_t)q.x & 15) == 0;
    a.vec_dx[o] = q.ld_dx % 4 == 0 && ((uintptr_t)q.dx & 15) == 0;
  }
  a.M = M; a.labels = labels; a.pixel_map = pixel_map; a.valid = nll_stats + valid_index; a.stats = stats_out;
  a.outputs = d->outputs; a.B = d->B; a.h = d->h; a.w = d->w; a.label_stride = d->label_stride;
  a.u = d->u; a.v = d->v; a.inv_fx = d->inv_fx; a.inv_fy = d->inv_fy;
  hipLaunchKernelGGL(reproj_loss_grad_kernel, dim3(1), dim3(RT), 0, reinterpret_cast<hipStream_t>(stream), a);
  KFN_LAUNCH_CHECK("reproj_loss_grad_kernel");
  return KFN_OK;
}
