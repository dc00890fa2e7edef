// kfn_train_filter.hip -- fine-tuning SCoordNet through the Kalman filter with OFlowNet frozen (gfx950): stage 3 of the
// reference's procedure under --fix_flownet (KFNet/train.py:268-298 with KFNet.GetKFCoordBatch, KFNet/KFNet.py:102-162).
// Compiled with -ffp-contract=off like kfn_train_loss.hip and kfn_kalman.hip: every product and sum is rounded as the
// reference's unfused TF elementwise ops are, and the sampler weights are bit for bit the forward scan's.
//   kfn_measurement_map   meas = (z, exp(log sigma)) from SCoordNet's raw output, the measurement the scan reads
//   kfn_filter_loss_grad  0.2 L_measure + 0.2 L_temporal + 0.6 L_KF: three times CoordLossWithUncertainty (KFNet/KFNet.py:192-232)
//                         + 50 SmoothLoss (:430-467), with the gradients with respect to the three outputs
//   kfn_filter_backward   the reverse scan t = T-1 .. 0: BuildKFCoord (:148-162), the variance chain (:393-401) and the
//                         transpose of tools.util.bilinear_sampler (tools/util.py:36-93) as a gather in a fixed order
//   kfn_filter_backward_joint  the same scan for joint stage 3 (OFlowNet trained too, KFNet/train.py:282-303): beside the above
//                         the gradients with respect to the flow (through the sampler's weights) and to sigma_trans
// The forward filter itself is kfn_kalman_scan_ex (kfn_kalman.hip): training and eval run the same launch.
#include "kfn_common.h"

#include <type_traits>

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

constexpr int LT = 1024;   // the loss is one workgroup, as kfn_coord_loss_grad is
constexpr int BT = 256;    // the backward scan: one thread per cell of a frame

__global__ __launch_bounds__(256) void measurement_map_kernel(const float* __restrict__ pred, int ld_pred, f32x4* __restrict__ meas,
                                                              long P) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= P) return;
  const float* x = pred + i * ld_pred;
  f32x4 z = {x[0], x[1], x[2], expf(x[3])};   // the same expf as the loss's sigma: one sigma_z per step
  meas[i] = z;
}

// ---- the loss ---------------------------------------------------------------------------------------------------------------
struct FilterLossArgs {
  const float* pred;
  const float* temp;
  const float* kf;
  const float* labels;
  const uint8_t* img;
  float* dpred;
  float* d_temp;
  float* d_kf;
  float* stats;
  int B, h, w, ld_pred, ld_dpred, label_stride, img_stride;
  int has_M, has_clip;
  float M[12];
  float clip, smooth_weight, thr2, min_unc;
  float weight[3];
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

// The three outputs are addressed alike: term k's map with its pixel stride, its gradient buffer with its own; the
// measurement's fourth channel is log sigma (EXP), the other two hold sigma itself.
struct Term {
  const float* x;
  float* g;
  int ldx, ldg;
  bool exp_sigma;
  float weight;
};

__global__ __launch_bounds__(LT) void filter_loss_grad_kernel(FilterLossArgs p) {
  __shared__ double red[LT];
  const int t = threadIdx.x;
  const long hw = (long)p.h * p.w, P = (long)p.B * hw;
  const int ls = p.label_stride, is = p.img_stride;
  const long lW = (long)p.w * ls, lH = (long)p.h * ls;   // label / image extents
  const long iW = (long)p.w * is, iH = (long)p.h * is;

  auto label_at = [&](int b, int r, int c) { return p.labels + (((long)b * lH + (long)r * ls) * lW + (long)c * ls) * 4; };
  auto mask_at = [&](int b, int r, int c) { return label_at(b, r, c)[3] == 1.0f ? 1.0f : 0.0f; };
  // exp(-0.625 * mean_c |img(a) - img(b)|) on the nearest-down-sampled frame (values 0..255)
  auto edge_weight = [&](int b, int r0, int c0, int r1, int c1) {
    const uint8_t* a = p.img + (((long)b * iH + (long)r0 * is) * iW + (long)c0 * is) * 3;
    const uint8_t* q = p.img + (((long)b * iH + (long)r1 * is) * iW + (long)c1 * is) * 3;
    const float s = (fabsf((float)a[0] - (float)q[0]) + fabsf((float)a[1] - (float)q[1])) + fabsf((float)a[2] - (float)q[2]);
    return expf(-0.625f * (s / 3.0f));
  };
  const Term terms[3] = {{p.pred, p.dpred, p.ld_pred, p.ld_dpred, true, p.weight[0]},
                         {p.temp, p.d_temp, 4, 4, false, p.weight[1]},
                         {p.kf, p.d_kf, 4, 4, false, p.weight[2]}};

  double cnt = 0.0;
  for (long i = t; i < P; i += LT) {
    const int b = (int)(i / hw);
    const int rem = (int)(i - b * hw);
    cnt += mask_at(b, rem / p.w, rem % p.w);
  }
  const float valid = (float)(block_sum(cnt, red) + 1.0);   // shared by the three terms, over the whole batch
  const bool smooth = p.smooth_weight != 0.0f;
  const float gs = p.smooth_weight * (2.0f / 3.0f) / valid;

  double s_nll[3] = {0.0, 0.0, 0.0}, s_smooth[3] = {0.0, 0.0, 0.0}, s_bad[3] = {0.0, 0.0, 0.0};
  for (long i = t; i < P; i += LT) {
    const int b = (int)(i / hw);
    const int rem = (int)(i - b * hw);
    const int r = rem / p.w, c = rem % p.w;
    const float* lab = label_at(b, r, c);
    const float m = lab[3] == 1.0f ? 1.0f : 0.0f;
    float g0 = lab[0], g1 = lab[1], g2 = lab[2];
    if (p.has_M) {   // gt = M [gt; 1]: ApplyTransform(gt, inv(transform.txt), inverse=True), KFNet/train.py:279-280
      const float a0 = ((p.M[0] * g0 + p.M[1] * g1) + p.M[2] * g2) + p.M[3];
      const float a1 = ((p.M[4] * g0 + p.M[5] * g1) + p.M[6] * g2) + p.M[7];
      const float a2 = ((p.M[8] * g0 + p.M[9] * g1) + p.M[10] * g2) + p.M[11];
      g0 = a0; g1 = a1; g2 = a2;
    }
    // the smoothness weights of this cell's four edges, never across a frame seam: (r, c) are positions inside frame b
    float w_right = 0.0f, w_left = 0.0f, w_down = 0.0f, w_up = 0.0f;
    if (smooth) {
      if (c + 1 < p.w) w_right = edge_weight(b, r, c, r, c + 1) * m;
      if (c > 0) w_left = edge_weight(b, r, c - 1, r, c) * mask_at(b, r, c - 1);
      if (r + 1 < p.h) w_down = edge_weight(b, r, c, r + 1, c) * m;
      if (r > 0) w_up = edge_weight(b, r - 1, c, r, c) * mask_at(b, r - 1, c);
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const Term& T = terms[k];
      const float* x = T.x + i * T.ldx;
      const float e0 = x[0] - g0, e1 = x[1] - g1, e2 = x[2] - g2;
      const float d = (e0 * e0 + e1 * e1) + e2 * e2;
      const float sigma = T.exp_sigma ? expf(x[3]) : x[3];
      const float u = fmaxf(sigma, p.min_unc);
      const float iu2 = 1.0f / (u * u);
      float l = 3.0f * logf(u) + d * 0.5f * iu2;
      float live = T.weight * (m / valid);   // d(L)/d(l) of this pixel
      if (p.has_clip && l > p.clip) {        // tf.minimum(loss_map, clip): no gradient through the constant
        l = p.clip;
        live = 0.0f;
      }
      s_nll[k] += (double)(m * l);
      s_bad[k] += (m * d - p.thr2 > 0.0f) ? 1.0 : 0.0;
      float gx0 = live * e0 * iu2, gx1 = live * e1 * iu2, gx2 = live * e2 * iu2;
      // through u = max(sigma, min) (gradient to sigma where sigma >= min) and, for the measurement, sigma = exp(ch3)
      float g3 = sigma >= p.min_unc ? live * (3.0f / u - d * iu2 / u) : 0.0f;
      if (T.exp_sigma) g3 = sigma >= p.min_unc ? live * (3.0f / u - d * iu2 / u) * sigma : 0.0f;

      if (smooth) {
        const float gk = T.weight * gs;
        float sm = 0.0f;
        if (c + 1 < p.w) {
          const float* y = x + T.ldx;
          const float q0 = x[0] - y[0], q1 = x[1] - y[1], q2 = x[2] - y[2];
          sm += ((q0 * q0 + q1 * q1) + q2 * q2) / 3.0f * w_right;
          gx0 += gk * w_right * q0; gx1 += gk * w_right * q1; gx2 += gk * w_right * q2;
        }
        if (c > 0) {
          const float* y = x - T.ldx;
          gx0 -= gk * w_left * (y[0] - x[0]); gx1 -= gk * w_left * (y[1] - x[1]); gx2 -= gk * w_left * (y[2] - x[2]);
        }
        if (r + 1 < p.h) {
          const float* y = x + (long)p.w * T.ldx;
          const float q0 = x[0] - y[0], q1 = x[1] - y[1], q2 = x[2] - y[2];
          sm += ((q0 * q0 + q1 * q1) + q2 * q2) / 3.0f * w_down;
          gx0 += gk * w_down * q0; gx1 += gk * w_down * q1; gx2 += gk * w_down * q2;
        }
        if (r > 0) {
          const float* y = x - (long)p.w * T.ldx;
          gx0 -= gk * w_up * (y[0] - x[0]); gx1 -= gk * w_up * (y[1] - x[1]); gx2 -= gk * w_up * (y[2] - x[2]);
        }
        s_smooth[k] += (double)sm;
      }
      float* g = T.g + i * T.ldg;
      g[0] = gx0; g[1] = gx1; g[2] = gx2; g[3] = g3;
    }
  }
  float term_total[3];
  for (int k = 0; k < 3; ++k) {
    const double nll = block_sum(s_nll[k], red);
    const double smo = block_sum(s_smooth[k], red);
    const double bad = block_sum(s_bad[k], red);
    const double v = (double)valid;
    term_total[k] = (float)(nll / v + (double)p.smooth_weight * (smo / v));
    if (t == 0) {
      p.stats[1 + k] = (float)(nll / v);
      p.stats[4 + k] = (float)(smo / v);
      p.stats[7 + k] = (float)((v - bad) / v);
      p.stats[12 + k] = term_total[k];
    }
  }
  if (t == 0) {
    // KFNet/train.py:293-295, fp32 like the graph's scalars
    p.stats[0] = (p.weight[0] * term_total[0] + p.weight[1] * term_total[1]) + p.weight[2] * term_total[2];
    p.stats[10] = valid;
    p.stats[15] = 0.0f;     // word 11 is kfn_filter_backward's
  }
}

// ---- the reverse scan ---------------------------------------------------------------------------------------------------------
struct BackArgs {
  const f32x2* flow;     // [S,T,hw]
  const f32x4* meas;     // [S,T,hw] (z, sigma_z)
  const f32x4* temp;     // [S,T,hw] (x^-, sigma^-)
  const f32x4* kf;       // [S,T,hw] (x, sigma)
  const f32x4* d_temp;   // [S,T,hw]
  f32x4* d_kf;           // [S,T,hw] in / out: on return the total gradient with respect to KF_t
  float* dpred;          // [S T hw, ld_dpred]: channels 0..3 += the filter's share
  f32x4* a_in;           // [S,hw] gradient with respect to frame t+1's sampled value, written by the launch before
  f32x4* a_out;          // [S,hw] the same for frame t
  unsigned* exceed;      // pixels of frames >= 1 whose flow leaves the radius
  int S, T, H, W, ld_dpred, radius, t;
  float eps2;
};

// What kfn_filter_backward_joint adds: the process noise it differentiates by, and its two outputs.
struct JointBackArgs : BackArgs {
  const float* sigma_trans;   // [S,T,hw]
  f32x2* d_flow;              // [S,T,hw] out
  float* d_sigma_trans;       // [S,T,hw] out
};

// The clamped corners and their weights of the target cell (x, y), exactly fuse_pixel's arithmetic (kfn_kalman.hip).
struct Taps {
  int ix0, ix1, iy0, iy1;
  float wx0, wx1, wy0, wy1;
};
__device__ __forceinline__ Taps taps_of(int x, int y, f32x2 flow, float xmax, float ymax) {
  const float px = (float)x + flow.x;
  const float py = (float)y + flow.y;
  const float x0 = floorf(px), x1 = x0 + 1.0f;
  const float y0 = floorf(py), y1 = y0 + 1.0f;
  const float x0s = fminf(fmaxf(x0, 0.f), xmax), x1s = fminf(fmaxf(x1, 0.f), xmax);
  const float y0s = fminf(fmaxf(y0, 0.f), ymax), y1s = fminf(fmaxf(y1, 0.f), ymax);
  Taps k;
  k.wx0 = x1s - px; k.wx1 = px - x0s;
  k.wy0 = y1s - py; k.wy1 = py - y0s;
  k.ix0 = (int)x0s; k.ix1 = (int)x1s; k.iy0 = (int)y0s; k.iy1 = (int)y1s;
  return k;
}

// One launch per frame t, last frame first; thread = source cell q of sequence s.
//   gather   (t < T-1) the transpose of frame t+1's sampler: q sums, rows then columns ascending, the contributions of the
//            target cells within radius + 1 of it, whose corners and weights are recomputed from the flow -- no atomics, so
//            the sum is the same in every launch; d_kf[t][q] += that sum
//   fuse     (t >= 1) d_temp[t], d_kf[t] -> the measurement's gradient (into dpred) and the gradient with respect to the
//            value sampled from KF_{t-1} (a_out, which the next launch gathers)
//   t == 0   d_temp[0] + d_kf[0] fall on the measurement
// JOINT (kfn_filter_backward_joint) adds, per cell of a frame t >= 1, the gradients with respect to the flow and to sigma_trans
// from values the fuse step holds already; frame 0 writes zeros to both.  The other instantiation is kfn_filter_backward's.
template <bool JOINT>
__global__ __launch_bounds__(BT) void filter_backward_kernel(std::conditional_t<JOINT, JointBackArgs, BackArgs> a) {
  const int HW = a.H * a.W;
  const int q = blockIdx.x * BT + threadIdx.x;
  const int s = blockIdx.y;
  if (q >= HW) return;
  const int t = a.t;
  const int qy = q / a.W, qx = q - qy * a.W;
  const float xmax = (float)(a.W - 1), ymax = (float)(a.H - 1);
  const size_t off = ((size_t)s * a.T + t) * HW;

  f32x4 G = a.d_kf[off + q];
  if (t < a.T - 1) {
    const f32x2* flow = a.flow + off + HW;           // frame t + 1
    const f32x4* ain = a.a_in + (size_t)s * HW;
    const int R = a.radius + 1;
    const int ylo = max(qy - R, 0), yhi = min(qy + R, a.H - 1);
    const int xlo = max(qx - R, 0), xhi = min(qx + R, a.W - 1);
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int y = ylo; y <= yhi; ++y) {
      for (int x = xlo; x <= xhi; ++x) {
        const int p = y * a.W + x;
        const Taps k = taps_of(x, y, flow[p], xmax, ymax);
        const bool hx0 = k.ix0 == qx, hx1 = k.ix1 == qx, hy0 = k.iy0 == qy, hy1 = k.iy1 == qy;
        if ((hx0 || hx1) && (hy0 || hy1)) {
          float c = 0.f;                              // the forward's add_n order: 00, 01, 10, 11
          if (hx0 && hy0) c += k.wx0 * k.wy0;
          if (hx0 && hy1) c += k.wx0 * k.wy1;
          if (hx1 && hy0) c += k.wx1 * k.wy0;
          if (hx1 && hy1) c += k.wx1 * k.wy1;
          acc += c * ain[p];
        }
      }
    }
    G += acc;
    a.d_kf[off + q] = G;
  }
  const f32x4 Gt = a.d_temp[off + q];
  const f32x4 z = a.meas[off + q];
  float* dp = a.dpred + (off + q) * a.ld_dpred;
  if (t == 0) {   // KFNet/KFNet.py:122-126: both estimates of frame 1 ARE the measurement
    const f32x4 gz = G + Gt;
    dp[0] += gz.x; dp[1] += gz.y; dp[2] += gz.z; dp[3] += gz.w * z.w;
    if constexpr (JOINT) {   // no pair ends on a group's first frame
      const f32x2 none = {0.f, 0.f};
      a.d_flow[off + q] = none;
      a.d_sigma_trans[off + q] = 0.0f;
    }
    return;
  }
  const f32x2 fl = a.flow[off + q];
  if (!(fabsf(fl.x) <= (float)a.radius && fabsf(fl.y) <= (float)a.radius)) atomicAdd(a.exceed, 1u);   // integer: order-free
  const f32x4 tp = a.temp[off + q];
  // BuildKFCoord backwards (KFNet/KFNet.py:148-162)
  const float lv = tp.w * tp.w, mv = z.w * z.w;
  const float sum = lv + mv;
  const float K = lv / sum;
  const float omr = 1.0f - K;
  const bool open = omr > 0.0f;                      // tf.maximum(1 - K, 0): both uses share the gate
  const float om = fmaxf(omr, 0.0f);
  const float sig = sqrtf(om * lv);
  const float dV = sig > 0.0f ? G.w / (2.0f * sig) : 0.0f;      // d / d(om * lv) through the square root
  const float d_om = ((G.x * tp.x + G.y * tp.y) + G.z * tp.z) + dV * lv;
  const float d_K = ((G.x * z.x + G.y * z.y) + G.z * z.z) - (open ? d_om : 0.0f);
  const float is2 = 1.0f / (sum * sum);
  const float d_lv = dV * om + d_K * mv * is2;
  const float d_mv = -(d_K * lv * is2);
  const float d_sm = d_lv * (2.0f * tp.w) + Gt.w;    // sigma^-: last_variance = square(sqrt(.)), plus the temporal term's own
  const float d_sz = d_mv * (2.0f * z.w);
  dp[0] += G.x * K; dp[1] += G.y * K; dp[2] += G.z * K; dp[3] += d_sz * z.w;
  // the variance chain (KFNet/KFNet.py:393-401): sigma^- = sqrt(max(s_l^2, eps^2) + max(sigma_trans^2, eps^2)); s_l is the
  // sample of KF_{t-1}'s sigma, recomputed with the forward's taps
  const Taps k = taps_of(qx, qy, fl, xmax, ymax);
  const f32x4* prev = a.kf + off - HW;
  const float s00 = prev[k.iy0 * a.W + k.ix0].w, s01 = prev[k.iy1 * a.W + k.ix0].w;
  const float s10 = prev[k.iy0 * a.W + k.ix1].w, s11 = prev[k.iy1 * a.W + k.ix1].w;
  const float s_l = (((k.wx0 * k.wy0) * s00 + (k.wx0 * k.wy1) * s01) + (k.wx1 * k.wy0) * s10) + (k.wx1 * k.wy1) * s11;
  const float d_lvar = d_sm / (2.0f * tp.w);
  f32x4 av;
  av.x = G.x * om + Gt.x; av.y = G.y * om + Gt.y; av.z = G.z * om + Gt.z;
  av.w = s_l * s_l > a.eps2 ? d_lvar * (2.0f * s_l) : 0.0f;     // below the floor the maximum passes nothing
  a.a_out[(size_t)s * HW + q] = av;
  if constexpr (JOINT) {
    // The sampler's weights are wx0 = x1s - px, wx1 = px - x0s (and likewise in y): their derivatives by (u, v) are -1 and +1,
    // the corner indices are piecewise constant (tools/util.py:36-59).  v_xy = corner (ix_x, iy_y) of KF_{t-1}.  Two corners
    // clamped to one cell hold the same value, so their difference is 0 by itself.  ORDER: channels 0..3 ascending.
    const f32x4 v00 = prev[k.iy0 * a.W + k.ix0], v01 = prev[k.iy1 * a.W + k.ix0];
    const f32x4 v10 = prev[k.iy0 * a.W + k.ix1], v11 = prev[k.iy1 * a.W + k.ix1];
    const f32x4 gu = k.wy0 * (v10 - v00) + k.wy1 * (v11 - v01);
    const f32x4 gv = k.wx0 * (v01 - v00) + k.wx1 * (v11 - v10);
    f32x2 df;
    df.x = ((av.x * gu.x + av.y * gu.y) + av.z * gu.z) + av.w * gu.w;
    df.y = ((av.x * gv.x + av.y * gv.y) + av.z * gv.z) + av.w * gv.w;
    a.d_flow[off + q] = df;
    // sigma^-^2 = max(s_l^2, eps^2) + max(sigma_trans^2, eps^2): the second maximum passes nothing below the floor
    const float st = a.sigma_trans[off + q];
    a.d_sigma_trans[off + q] = st * st > a.eps2 ? d_lvar * (2.0f * st) : 0.0f;
  }
}

}  // namespace

extern "C" int kfn_measurement_map(const float* pred, int ld_pred, float* meas, long pixels, void* stream) {
  KFN_REQUIRE(pred && meas && pixels > 0 && ld_pred >= 4, "kfn_measurement_map: bad argument");
  KFN_REQUIRE((reinterpret_cast<uintptr_t>(meas) & 15) == 0, "kfn_measurement_map: meas must be 16-byte aligned");
  const long blocks = (pixels + 255) / 256;
  KFN_REQUIRE(blocks < (1L << 31), "kfn_measurement_map: %ld pixels are too many for one launch", pixels);
  hipLaunchKernelGGL(measurement_map_kernel, dim3((unsigned)blocks), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), pred,
                     ld_pred, reinterpret_cast<f32x4*>(meas), pixels);
  KFN_LAUNCH_CHECK("measurement_map_kernel");
  return KFN_OK;
}

extern "C" int kfn_filter_loss_grad(const kfn_filter_loss_desc* d, const float* pred, const float* temp, const float* kf,
                                    const float* labels, const uint8_t* img, float* dpred, float* d_temp, float* d_kf,
                                    float* stats, void* stream) {
  KFN_REQUIRE(d && pred && temp && kf && labels && dpred && d_temp && d_kf && stats, "kfn_filter_loss_grad: null argument");
  KFN_REQUIRE(d->struct_size == (int32_t)sizeof(kfn_filter_loss_desc), "kfn_filter_loss_grad: struct_size %d, expected %d",
              (int)d->struct_size, (int)sizeof(kfn_filter_loss_desc));
  KFN_REQUIRE(d->B > 0 && d->h > 0 && d->w > 0 && (long)d->B * d->h * d->w < (1L << 24),
              "kfn_filter_loss_grad: bad grid %dx%dx%d", d->B, d->h, d->w);
  KFN_REQUIRE(d->ld_pred >= 4 && d->ld_dpred >= 4, "kfn_filter_loss_grad: pixel strides below 4 (%d, %d)", d->ld_pred, d->ld_dpred);
  KFN_REQUIRE(d->label_stride >= 1 && d->img_stride >= 1, "kfn_filter_loss_grad: bad label_stride %d / img_stride %d",
              d->label_stride, d->img_stride);
  KFN_REQUIRE(d->smooth_weight == 0.0f || img, "kfn_filter_loss_grad: the smoothness term needs the frames");
  KFN_REQUIRE(d->min_uncertainty > 0.0 && d->dist_threshold >= 0.0, "kfn_filter_loss_grad: bad thresholds");
  FilterLossArgs a;
  a.pred = pred; a.temp = temp; a.kf = kf; a.labels = labels; a.img = img;
  a.dpred = dpred; a.d_temp = d_temp; a.d_kf = d_kf; a.stats = stats;
  a.B = d->B; a.h = d->h; a.w = d->w; a.ld_pred = d->ld_pred; a.ld_dpred = d->ld_dpred;
  a.label_stride = d->label_stride; a.img_stride = d->img_stride;
  a.has_M = d->has_transform; a.has_clip = d->has_loss_clip;
  for (int i = 0; i < 12; ++i) a.M[i] = d->transform[i];
  a.clip = d->loss_clip; a.smooth_weight = d->smooth_weight;
  // the reference squares the Python double and TensorFlow rounds the product once (KFNet/KFNet.py:227): 0x3B23D70A for 0.05
  a.thr2 = (float)(d->dist_threshold * d->dist_threshold); a.min_unc = (float)d->min_uncertainty;
  a.weight[0] = d->weight_measure; a.weight[1] = d->weight_temporal; a.weight[2] = d->weight_kf;
  hipLaunchKernelGGL(filter_loss_grad_kernel, dim3(1), dim3(LT), 0, reinterpret_cast<hipStream_t>(stream), a);
  KFN_LAUNCH_CHECK("filter_loss_grad_kernel");
  return KFN_OK;
}

extern "C" int kfn_filter_backward_scratch_bytes(const kfn_filter_backward_desc* d, size_t* bytes) {
  KFN_REQUIRE(d && bytes, "kfn_filter_backward_scratch_bytes: null argument");
  KFN_REQUIRE(d->S > 0 && d->H > 1 && d->W > 1, "kfn_filter_backward_scratch_bytes: bad shape S=%d H=%d W=%d", d->S, d->H, d->W);
  *bytes = 2 * (size_t)d->S * d->H * d->W * sizeof(f32x4);      // the sampled value's gradient of two consecutive frames
  return KFN_OK;
}

extern "C" int kfn_filter_backward(const kfn_filter_backward_desc* d, const float* flow_xy, const float* meas, const float* temp,
                                   const float* kf, const float* d_temp, float* d_kf, float* dpred, float* stats, void* scratch,
                                   void* stream) {
  KFN_REQUIRE(d && flow_xy && meas && temp && kf && d_temp && d_kf && dpred && stats && scratch, "kfn_filter_backward: null argument");
  KFN_REQUIRE(d->struct_size == (int32_t)sizeof(kfn_filter_backward_desc), "kfn_filter_backward: struct_size %d, expected %d",
              (int)d->struct_size, (int)sizeof(kfn_filter_backward_desc));
  KFN_REQUIRE(d->S > 0 && d->S < 65536 && d->T > 0 && d->H > 1 && d->W > 1 && (long)d->S * d->T * d->H * d->W < (1L << 27),
              "kfn_filter_backward: bad shape S=%d T=%d H=%d W=%d", d->S, d->T, d->H, d->W);
  KFN_REQUIRE(d->radius >= 4 && d->radius <= 64, "kfn_filter_backward: radius %d outside 4..64", d->radius);
  KFN_REQUIRE(d->ld_dpred >= 4 && d->min_uncertainty > 0.0, "kfn_filter_backward: bad ld_dpred %d or min_uncertainty", d->ld_dpred);
  KFN_REQUIRE(((reinterpret_cast<uintptr_t>(flow_xy) & 7) |
               ((reinterpret_cast<uintptr_t>(meas) | reinterpret_cast<uintptr_t>(temp) | reinterpret_cast<uintptr_t>(kf) |
                 reinterpret_cast<uintptr_t>(d_temp) | reinterpret_cast<uintptr_t>(d_kf) | reinterpret_cast<uintptr_t>(scratch)) & 15)) == 0,
              "kfn_filter_backward: misaligned buffer");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int HW = d->H * d->W;
  BackArgs a;
  a.flow = reinterpret_cast<const f32x2*>(flow_xy);
  a.meas = reinterpret_cast<const f32x4*>(meas);
  a.temp = reinterpret_cast<const f32x4*>(temp);
  a.kf = reinterpret_cast<const f32x4*>(kf);
  a.d_temp = reinterpret_cast<const f32x4*>(d_temp);
  a.d_kf = reinterpret_cast<f32x4*>(d_kf);
  a.dpred = dpred;
  a.exceed = reinterpret_cast<unsigned*>(stats + 11);
  a.S = d->S; a.T = d->T; a.H = d->H; a.W = d->W; a.ld_dpred = d->ld_dpred; a.radius = d->radius;
  a.eps2 = (float)(d->min_uncertainty * d->min_uncertainty);   // the scan's floor_variance: the double product rounded once
  f32x4* buf[2] = {reinterpret_cast<f32x4*>(scratch), reinterpret_cast<f32x4*>(scratch) + (size_t)d->S * HW};
  KFN_HIP(hipMemsetAsync(a.exceed, 0, sizeof(unsigned), s));
  const dim3 grid((unsigned)((HW + BT - 1) / BT), (unsigned)d->S);
  // T stream-ordered launches instead of one workgroup per sequence: a step trains one or a few groups, and a frame's cells
  // are independent once the frame after it is done, so each launch spreads S H W threads over the chip.
  for (int t = d->T - 1; t >= 0; --t) {
    a.t = t;
    a.a_out = buf[t & 1];
    a.a_in = buf[(t + 1) & 1];
    hipLaunchKernelGGL(filter_backward_kernel<false>, grid, dim3(BT), 0, s, a);
    KFN_LAUNCH_CHECK("filter_backward_kernel");
  }
  return KFN_OK;
}

extern "C" int kfn_filter_backward_joint(const kfn_filter_backward_desc* d, const float* flow_xy, const float* sigma_trans,
                                         const float* meas, const float* temp, const float* kf, const float* d_temp, float* d_kf,
                                         float* dpred, float* d_flow, float* d_sigma_trans, float* stats, void* scratch,
                                         void* stream) {
  KFN_REQUIRE(d && flow_xy && sigma_trans && meas && temp && kf && d_temp && d_kf && dpred && d_flow && d_sigma_trans && stats &&
              scratch, "kfn_filter_backward_joint: null argument");
  KFN_REQUIRE(d->struct_size == (int32_t)sizeof(kfn_filter_backward_desc), "kfn_filter_backward_joint: struct_size %d, expected %d",
              (int)d->struct_size, (int)sizeof(kfn_filter_backward_desc));
  KFN_REQUIRE(d->S > 0 && d->S < 65536 && d->T > 0 && d->H > 1 && d->W > 1 && (long)d->S * d->T * d->H * d->W < (1L << 27),
              "kfn_filter_backward_joint: bad shape S=%d T=%d H=%d W=%d", d->S, d->T, d->H, d->W);
  KFN_REQUIRE(d->radius >= 4 && d->radius <= 64, "kfn_filter_backward_joint: radius %d outside 4..64", d->radius);
  KFN_REQUIRE(d->ld_dpred >= 4 && d->min_uncertainty > 0.0, "kfn_filter_backward_joint: bad ld_dpred %d or min_uncertainty",
              d->ld_dpred);
  KFN_REQUIRE((((reinterpret_cast<uintptr_t>(flow_xy) | reinterpret_cast<uintptr_t>(d_flow)) & 7) |
               ((reinterpret_cast<uintptr_t>(sigma_trans) | reinterpret_cast<uintptr_t>(d_sigma_trans)) & 3) |
               ((reinterpret_cast<uintptr_t>(meas) | reinterpret_cast<uintptr_t>(temp) | reinterpret_cast<uintptr_t>(kf) |
                 reinterpret_cast<uintptr_t>(d_temp) | reinterpret_cast<uintptr_t>(d_kf) | reinterpret_cast<uintptr_t>(scratch)) & 15)) == 0,
              "kfn_filter_backward_joint: misaligned buffer");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int HW = d->H * d->W;
  JointBackArgs a;
  a.flow = reinterpret_cast<const f32x2*>(flow_xy);
  a.meas = reinterpret_cast<const f32x4*>(meas);
  a.temp = reinterpret_cast<const f32x4*>(temp);
  a.kf = reinterpret_cast<const f32x4*>(kf);
  a.d_temp = reinterpret_cast<const f32x4*>(d_temp);
  a.d_kf = reinterpret_cast<f32x4*>(d_kf);
  a.dpred = dpred;
  a.exceed = reinterpret_cast<unsigned*>(stats + 11);
  a.S = d->S; a.T = d->T; a.H = d->H; a.W = d->W; a.ld_dpred = d->ld_dpred; a.radius = d->radius;
  a.eps2 = (float)(d->min_uncertainty * d->min_uncertainty);
  a.sigma_trans = sigma_trans;
  a.d_flow = reinterpret_cast<f32x2*>(d_flow);
  a.d_sigma_trans = d_sigma_trans;
  f32x4* buf[2] = {reinterpret_cast<f32x4*>(scratch), reinterpret_cast<f32x4*>(scratch) + (size_t)d->S * HW};
  KFN_HIP(hipMemsetAsync(a.exceed, 0, sizeof(unsigned), s));
  const dim3 grid((unsigned)((HW + BT - 1) / BT), (unsigned)d->S);
  for (int t = d->T - 1; t >= 0; --t) {   // the launches of kfn_filter_backward, frame for frame
    a.t = t;
    a.a_out = buf[t & 1];
    a.a_in = buf[(t + 1) & 1];
    hipLaunchKernelGGL(filter_backward_kernel<true>, grid, dim3(BT), 0, s, a);
    KFN_LAUNCH_CHECK("filter_backward_kernel<joint>");
  }
  return KFN_OK;
}
