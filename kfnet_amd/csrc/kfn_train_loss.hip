// kfn_train_loss.hip -- SCoordNet's training loss with its gradient, and TensorFlow's Adam update (gfx950).
// Compiled with -ffp-contract=off like kfn_metrics.hip: the loss restates TF elementwise ops whose results are clipped,
// thresholded and counted.
//   kfn_coord_loss_grad  KFNet.MeasureCoordLoss restricted to the measurement term: CoordLossWithUncertainty
//                        (KFNet/KFNet.py:192-232) + 50 * SmoothLoss (:250-252, :430-467) on the labels of KFNet/train.py:
//                        274-280, and d(loss)/d(prediction) -- what tf.gradients hands to the last convolution.
//   kfn_adam_step        tf.train.AdamOptimizer (KFNet/train.py:313) with the L2 regulariser's gradient (:301-303) folded in.
#include "kfn_common.h"

namespace {

constexpr int LT = 1024;   // one workgroup: the grid is H/8 x W/8 per frame, a few 10^4 pixels per batch

struct LossArgs {
  const float* pred;
  const float* labels;
  const uint8_t* img;
  float* dpred;
  float* stats;
  int B, h, w, ld_pred, ld_dpred, label_stride, img_stride;
  int has_M, has_clip;
  float M[12];
  float clip, smooth_weight, thr2, min_unc;
};

__device__ __forceinline__ double block_sum(double v, double* red) {
  const int t = threadIdx.x;
  __syncthreads();
  red[t] = v;
  __syncthreads();
  for (int s = LT / 2; s > 0; s >>= 1) {   // a fixed tree: the same sum in every launch
    if (t < s) red[t] += red[t + s];
    __syncthreads();
  }
  return red[0];
}

__global__ __launch_bounds__(LT) void coord_loss_grad_kernel(LossArgs p) {
  __shared__ double red[LT];
  const int t = threadIdx.x;
  const long hw = (long)p.h * p.w, P = (long)p.B * hw;
  const int ls = p.label_stride, is = p.img_stride;
  const long lW = (long)p.w * ls, lH = (long)p.h * ls;   // label / image extents
  const long iW = (long)p.w * is, iH = (long)p.h * is;

  auto label_at = [&](int b, int r, int c) { return p.labels + (((long)b * lH + (long)r * ls) * lW + (long)c * ls) * 4; };
  auto mask_at = [&](int b, int r, int c) { return label_at(b, r, c)[3] == 1.0f ? 1.0f : 0.0f; };
  auto pred_at = [&](int b, int r, int c) { return p.pred + (((long)b * p.h + r) * p.w + c) * p.ld_pred; };
  // exp(-0.625 * mean_c |img(a) - img(b)|) on the nearest-down-sampled frame (values 0..255)
  auto edge_weight = [&](int b, int r0, int c0, int r1, int c1) {
    const uint8_t* a = p.img + (((long)b * iH + (long)r0 * is) * iW + (long)c0 * is) * 3;
    const uint8_t* q = p.img + (((long)b * iH + (long)r1 * is) * iW + (long)c1 * is) * 3;
    const float s = (fabsf((float)a[0] - (float)q[0]) + fabsf((float)a[1] - (float)q[1])) + fabsf((float)a[2] - (float)q[2]);
    return expf(-0.625f * (s / 3.0f));
  };

  double cnt = 0.0;
  for (long i = t; i < P; i += LT) {
    const int b = (int)(i / hw);
    const int rem = (int)(i - b * hw);
    cnt += mask_at(b, rem / p.w, rem % p.w);
  }
  const float valid = (float)(block_sum(cnt, red) + 1.0);
  const bool smooth = p.smooth_weight != 0.0f;
  const float gs = p.smooth_weight * (2.0f / 3.0f) / valid;

  double s_nll = 0.0, s_smooth = 0.0, s_bad = 0.0;
  for (long i = t; i < P; i += LT) {
    const int b = (int)(i / hw);
    const int rem = (int)(i - b * hw);
    const int r = rem / p.w, c = rem % p.w;
    const float* x = pred_at(b, r, c);
    const float* lab = label_at(b, r, c);
    const float m = lab[3] == 1.0f ? 1.0f : 0.0f;
    float g0 = lab[0], g1 = lab[1], g2 = lab[2];
    if (p.has_M) {   // gt = M [gt; 1]: ApplyTransform(gt, inv(transform.txt), inverse=True), KFNet/train.py:279-280
      const float a0 = ((p.M[0] * g0 + p.M[1] * g1) + p.M[2] * g2) + p.M[3];
      const float a1 = ((p.M[4] * g0 + p.M[5] * g1) + p.M[6] * g2) + p.M[7];
      const float a2 = ((p.M[8] * g0 + p.M[9] * g1) + p.M[10] * g2) + p.M[11];
      g0 = a0; g1 = a1; g2 = a2;
    }
    const float e0 = x[0] - g0, e1 = x[1] - g1, e2 = x[2] - g2;
    const float d = (e0 * e0 + e1 * e1) + e2 * e2;
    const float sigma = expf(x[3]);
    const float u = fmaxf(sigma, p.min_unc);
    const float iu2 = 1.0f / (u * u);
    float l = 3.0f * logf(u) + d * 0.5f * iu2;
    float live = m / valid;            // d(loss)/d(l) of this pixel
    if (p.has_clip && l > p.clip) {    // tf.minimum(loss_map, clip): no gradient through the constant
      l = p.clip;
      live = 0.0f;
    }
    s_nll += (double)(m * l);
    s_bad += (m * d - p.thr2 > 0.0f) ? 1.0 : 0.0;
    float gx0 = live * e0 * iu2, gx1 = live * e1 * iu2, gx2 = live * e2 * iu2;
    // through u = max(sigma, min) (gradient to sigma where sigma >= min) and sigma = exp(ch3)
    const float g3 = sigma >= p.min_unc ? live * (3.0f / u - d * iu2 / u) * sigma : 0.0f;

    if (smooth) {
      float sm = 0.0f;
      if (c + 1 < p.w) {
        const float* y = pred_at(b, r, c + 1);
        const float wgt = edge_weight(b, r, c, r, c + 1) * m;
        const float q0 = x[0] - y[0], q1 = x[1] - y[1], q2 = x[2] - y[2];
        sm += ((q0 * q0 + q1 * q1) + q2 * q2) / 3.0f * wgt;
        gx0 += gs * wgt * q0; gx1 += gs * wgt * q1; gx2 += gs * wgt * q2;
      }
      if (c > 0) {
        const float* y = pred_at(b, r, c - 1);
        const float wgt = edge_weight(b, r, c - 1, r, c) * mask_at(b, r, c - 1);
        gx0 -= gs * wgt * (y[0] - x[0]); gx1 -= gs * wgt * (y[1] - x[1]); gx2 -= gs * wgt * (y[2] - x[2]);
      }
      if (r + 1 < p.h) {
        const float* y = pred_at(b, r + 1, c);
        const float wgt = edge_weight(b, r, c, r + 1, c) * m;
        const float q0 = x[0] - y[0], q1 = x[1] - y[1], q2 = x[2] - y[2];
        sm += ((q0 * q0 + q1 * q1) + q2 * q2) / 3.0f * wgt;
        gx0 += gs * wgt * q0; gx1 += gs * wgt * q1; gx2 += gs * wgt * q2;
      }
      if (r > 0) {
        const float* y = pred_at(b, r - 1, c);
        const float wgt = edge_weight(b, r - 1, c, r, c) * mask_at(b, r - 1, c);
        gx0 -= gs * wgt * (y[0] - x[0]); gx1 -= gs * wgt * (y[1] - x[1]); gx2 -= gs * wgt * (y[2] - x[2]);
      }
      s_smooth += (double)sm;
    }
    float* g = p.dpred + i * p.ld_dpred;
    g[0] = gx0; g[1] = gx1; g[2] = gx2; g[3] = g3;
  }
  const double nll = block_sum(s_nll, red);
  const double smo = block_sum(s_smooth, red);
  const double bad = block_sum(s_bad, red);
  if (t == 0) {
    const double v = (double)valid;
    p.stats[0] = (float)(nll / v);
    p.stats[1] = (float)(smo / v);
    p.stats[2] = (float)((v - bad) / v);
    p.stats[3] = valid;
    p.stats[4] = (float)(nll / v + (double)p.smooth_weight * (smo / v));
    p.stats[5] = p.stats[6] = p.stats[7] = 0.0f;
  }
}

// Arithmetic in fp64, one rounding per stored value: m, v and w are fp32 variables as in TensorFlow.
__global__ __launch_bounds__(256) void adam_step_kernel(float* __restrict__ w, float* __restrict__ m, float* __restrict__ v,
                                                        const float* __restrict__ g, long n, double lr_t, double b1, double b2,
                                                        double eps, double wd) {
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

}  // namespace

extern "C" int kfn_coord_loss_grad(const kfn_coord_loss_desc* d, const float* pred, const float* labels, const uint8_t* img,
                                   float* dpred, float* stats, void* stream) {
  KFN_REQUIRE(d && pred && labels && dpred && stats, "kfn_coord_loss_grad: null argument");
  KFN_REQUIRE(d->struct_size == (int32_t)sizeof(kfn_coord_loss_desc), "kfn_coord_loss_grad: struct_size %d, expected %d",
              (int)d->struct_size, (int)sizeof(kfn_coord_loss_desc));
  KFN_REQUIRE(d->B > 0 && d->h > 0 && d->w > 0 && (long)d->B * d->h * d->w < (1L << 24),
              "kfn_coord_loss_grad: bad grid %dx%dx%d", d->B, d->h, d->w);
  KFN_REQUIRE(d->ld_pred >= 4 && d->ld_dpred >= 4, "kfn_coord_loss_grad: pixel strides below 4 (%d, %d)", d->ld_pred, d->ld_dpred);
  KFN_REQUIRE(d->label_stride >= 1 && d->img_stride >= 1, "kfn_coord_loss_grad: bad label_stride %d / img_stride %d",
              d->label_stride, d->img_stride);
  KFN_REQUIRE(d->smooth_weight == 0.0f || img, "kfn_coord_loss_grad: the smoothness term needs the frames");
  KFN_REQUIRE(d->min_uncertainty > 0.0 && d->dist_threshold >= 0.0, "kfn_coord_loss_grad: bad thresholds");
  LossArgs a;
  a.pred = pred; a.labels = labels; a.img = img; a.dpred = dpred; a.stats = stats;
  a.B = d->B; a.h = d->h; a.w = d->w; a.ld_pred = d->ld_pred; a.ld_dpred = d->ld_dpred;
  a.label_stride = d->label_stride; a.img_stride = d->img_stride;
  a.has_M = d->has_transform; a.has_clip = d->has_loss_clip;
  for (int i = 0; i < 12; ++i) a.M[i] = d->transform[i];
  a.clip = d->loss_clip; a.smooth_weight = d->smooth_weight;
  // the reference squares the Python double and TensorFlow rounds the product once (KFNet/KFNet.py:227): 0x3B23D70A for 0.05
  a.thr2 = (float)(d->dist_threshold * d->dist_threshold); a.min_unc = (float)d->min_uncertainty;
  hipLaunchKernelGGL(coord_loss_grad_kernel, dim3(1), dim3(LT), 0, reinterpret_cast<hipStream_t>(stream), a);
  KFN_LAUNCH_CHECK("coord_loss_grad_kernel");
  return KFN_OK;
}

extern "C" int kfn_adam_step(float* w, float* m, float* v, const float* g, long n, double lr_t, double beta1, double beta2,
                             double epsilon, double weight_decay, void* stream) {
  KFN_REQUIRE(w && m && v && g, "kfn_adam_step: null argument");
  KFN_REQUIRE(n > 0, "kfn_adam_step: n = %ld", n);
  KFN_REQUIRE(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0 && epsilon > 0.0 && weight_decay >= 0.0 && lr_t == lr_t,
              "kfn_adam_step: bad hyper-parameters");
  long blocks = (n + 255) / 256;
  if (blocks > 16384) blocks = 16384;
  hipLaunchKernelGGL(adam_step_kernel, dim3((unsigned)blocks), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), w, m, v, g, n,
                     lr_t, beta1, beta2, epsilon, weight_decay);
  KFN_LAUNCH_CHECK("adam_step_kernel");
  return KFN_OK;
}
