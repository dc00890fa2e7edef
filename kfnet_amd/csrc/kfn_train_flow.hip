// kfn_train_flow.hip -- training OFlowNet (stage 2 of the reference's procedure): the backward launches of the Temporal scope
// that are not convolutions, and the loss (gfx950).
// Compiled with -ffp-contract=off like kfn_train_filter.hip: the loss's per-cell terms and the sampler weights are rounded as
// the forward's unfused elementwise ops are, and the two gather sums are plain sequential fp32 additions.
//   kfn_cost_volume_backward  the transpose of KFNet.BuildCoordVolume (KFNet/KFNet.py:343-359): d_vol -> (d_f2, d_f1)
//   kfn_flow_head_backward    OFlowNet.GetOutput's softmax (cnn_wrapper/OFlowNet.py:45-47) with BuildOFlowNet's soft-argmax
//                             (KFNet/KFNet.py:381-385), and exp(.) 1e-2 of the process noise (OFlowNet.py:56)
//   kfn_l2norm_backward       tf.nn.l2_normalize over the 32 channels of feat7 (KFNet/KFNet.py:335-338)
//   kfn_flow_loss_grad        the prior loss: CoordLossWithUncertainty (KFNet/KFNet.py:192-232) of label a warped by the flow
//                             (tools/util.py:36-93) against label b, the process noise as uncertainty
// No floating-point atomics: every sum has a fixed order, two launches give the same bits.
#include "kfn_common.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int LT = 1024;      // the loss is one workgroup, as kfn_coord_loss_grad is
constexpr int WINDOW = 8;     // the cost volume's window and the soft-argmax's: offsets -4..3
constexpr int CELLS = WINDOW * WINDOW;

// ---- the cost volume ------------------------------------------------------------------------------------------------------
// Thread = (which output, cell, channel quad): the C/4 lanes of a cell read one contiguous run of C floats per (i, j), 64
// times, so every read of a wave is whole 16 C-byte runs (a full 128-byte line at C = 32).  Cells are i, j ascending.
__global__ __launch_bounds__(256) void cost_volume_backward_kernel(const f32x4* __restrict__ d_vol, f32x4* __restrict__ d_f2,
                                                                   f32x4* __restrict__ d_f1, int N, int H, int W, int C4) {
  const long cells = (long)N * H * W;
  const long per_output = cells * C4;
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= 2 * per_output) return;
  const bool to_f1 = idx >= per_output;            // the second half of the grid gathers d_f1
  const long e = to_f1 ? idx - per_output : idx;
  const long cell = e / C4;
  const int c4 = (int)(e - cell * C4);
  const long window_stride = (long)CELLS * C4;     // quads per cell of d_vol
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  if (!to_f1) {
    const f32x4* src = d_vol + cell * window_stride + c4;
#pragma unroll 8
    for (int k = 0; k < CELLS; ++k) acc += src[(long)k * C4];
    d_f2[e] = acc;
    return;
  }
  const int x = (int)(cell % W);
  const long rest = cell / W;
  const int y = (int)(rest % H);
  const long n = rest / H;
  for (int i = 0; i < WINDOW; ++i) {
    const int sy = y - (i - WINDOW / 2);           // the cell whose window holds q at row i
    if ((unsigned)sy >= (unsigned)H) continue;
    for (int j = 0; j < WINDOW; ++j) {
      const int sx = x - (j - WINDOW / 2);
      if ((unsigned)sx >= (unsigned)W) continue;
      const long p = (n * H + sy) * W + sx;
      acc += d_vol[p * window_stride + (long)(i * WINDOW + j) * C4 + c4];
    }
  }
  d_f1[e] = -acc;
}

// ---- the flow head ---------------------------------------------------------------------------------------------------------
// One wave per window, lane k = cell (i, j) = (k / 8, k % 8) with offset o_k = (j - 4, i - 4).
__global__ __launch_bounds__(256) void flow_head_backward_kernel(const float* __restrict__ d_flow, const float* __restrict__ prob,
                                                                 const float* __restrict__ d_sigma,
                                                                 const float* __restrict__ sigma_trans, float* __restrict__ d_logits,
                                                                 int ld_logits, float* __restrict__ d_pre, int ld_pre, long N) {
  const int lane = threadIdx.x & 63;
  const long n = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (n >= N) return;                                // wave-uniform
  const float gx = d_flow[2 * n], gy = d_flow[2 * n + 1];
  const float pk = prob[n * CELLS + lane];
  const float sk = (float)((lane & 7) - WINDOW / 2) * gx + (float)((lane >> 3) - WINDOW / 2) * gy;
  const float mean = kfn::wave_sum_dpp(pk * sk);     // a fixed tree over the 64 lanes
  const float dl = pk * (sk - mean);
  // the window's 64 rows of ld_logits floats are one contiguous run: lanes store consecutive quads of it
  const int q_per_row = ld_logits >> 2;
  f32x4* out = reinterpret_cast<f32x4*>(d_logits + n * CELLS * ld_logits);
  for (int q = lane; q < CELLS * q_per_row; q += 64) {
    const int row = q / q_per_row;
    const float v = __shfl(dl, row);
    f32x4 o = {0.f, 0.f, 0.f, 0.f};
    if (q - row * q_per_row == 0) o.x = v;
    out[q] = o;
  }
  if (lane < ld_pre) d_pre[n * ld_pre + lane] = lane == 0 ? d_sigma[n] * sigma_trans[n] : 0.0f;
}

// ---- the L2 normalisation --------------------------------------------------------------------------------------------------
// y = x rsqrt(max(sum x^2, 1e-12)) over 32 channels: eight lanes per pixel, a quad of channels each, sums over a fixed
// butterfly inside the eight lanes.
__device__ __forceinline__ float sum8(float v) {
  v += __shfl_xor(v, 1);
  v += __shfl_xor(v, 2);
  v += __shfl_xor(v, 4);
  return v;
}

__global__ __launch_bounds__(256) void l2norm_backward_kernel(const float* __restrict__ x, int ldx, const float* __restrict__ g,
                                                              int ldg, float* __restrict__ dx, int ld_dx, long P) {
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  const long p = t >> 3;
  const int c = (int)(t & 7) * 4;
  const bool live = p < P;                           // the shuffles need every lane of the wave
  f32x4 xv = {0.f, 0.f, 0.f, 0.f}, gv = {0.f, 0.f, 0.f, 0.f};
  if (live) {
    xv = *reinterpret_cast<const f32x4*>(x + p * ldx + c);
    gv = *reinterpret_cast<const f32x4*>(g + p * ldg + c);
  }
  const float ss = sum8((xv.x * xv.x + xv.y * xv.y) + (xv.z * xv.z + xv.w * xv.w));
  const bool above = ss > 1e-12f;                     // under the floor the factor is the constant rsqrt(1e-12)
  const float r = above ? 1.0f / sqrtf(ss) : 1e6f;
  const f32x4 yv = xv * r;
  const float yg = sum8((yv.x * gv.x + yv.y * gv.y) + (yv.z * gv.z + yv.w * gv.w));
  const f32x4 o = above ? (gv - yv * yg) * r : gv * r;
  if (live) *reinterpret_cast<f32x4*>(dx + p * ld_dx + c) = o;
}

// ---- the loss ----------------------------------------------------------------------------------------------------------------
struct FlowLossArgs {
  const float* flow;
  const float* sigma_trans;
  const float* labels;
  float* d_flow;
  float* d_sigma;
  float* stats;
  int P, h, w, label_stride, has_clip;
  float clip, thr2, min_unc, eps2;
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

// What a cell of pair p needs from label a: the sampler's clamped corners with their weights (kfn_kalman.hip's fuse_pixel
// arithmetic, tools/util.py:36-93) and whether the four UNCLAMPED corners lie in the grid.
struct Warp {
  int ix0, ix1, iy0, iy1;
  float wx0, wx1, wy0, wy1;
  bool inside;
};
__device__ __forceinline__ Warp warp_of(int x, int y, float u, float v, int w, int h) {
  const float xmax = (float)(w - 1), ymax = (float)(h - 1);
  const float px = (float)x + u;
  const float py = (float)y + v;
  const float x0 = floorf(px), x1 = x0 + 1.0f;
  const float y0 = floorf(py), y1 = y0 + 1.0f;
  const float x0s = fminf(fmaxf(x0, 0.f), xmax), x1s = fminf(fmaxf(x1, 0.f), xmax);
  const float y0s = fminf(fmaxf(y0, 0.f), ymax), y1s = fminf(fmaxf(y1, 0.f), ymax);
  Warp k;
  k.wx0 = x1s - px; k.wx1 = px - x0s;
  k.wy0 = y1s - py; k.wy1 = py - y0s;
  k.ix0 = (int)x0s; k.ix1 = (int)x1s; k.iy0 = (int)y0s; k.iy1 = (int)y1s;
  k.inside = x0 >= 0.f && x1 <= xmax && y0 >= 0.f && y1 <= ymax;   // false for NaN too
  return k;
}

__global__ __launch_bounds__(LT) void flow_loss_grad_kernel(FlowLossArgs p) {
  __shared__ double red[LT];
  const int t = threadIdx.x;
  const long hw = (long)p.h * p.w, cells = (long)p.P * hw;
  const int ls = p.label_stride;
  const long lW = (long)p.w * ls, lH = (long)p.h * ls;
  // frame 2 pair is a, frame 2 pair + 1 is b
  auto label_at = [&](long frame, int r, int c) { return p.labels + ((frame * lH + (long)r * ls) * lW + (long)c * ls) * 4; };

  // M = m_b valid_a of a cell, with the warp it was decided on
  auto mask_of = [&](long i, Warp* k, float* valid_a) {
    const long pair = i / hw;
    const int rem = (int)(i - pair * hw);
    const int r = rem / p.w, c = rem - r * p.w;
    *k = warp_of(c, r, p.flow[2 * i], p.flow[2 * i + 1], p.w, p.h);
    float va = 0.0f;
    if (k->inside) {
      const long a = 2 * pair;
      va = (label_at(a, k->iy0, k->ix0)[3] == 1.0f && label_at(a, k->iy1, k->ix0)[3] == 1.0f &&
            label_at(a, k->iy0, k->ix1)[3] == 1.0f && label_at(a, k->iy1, k->ix1)[3] == 1.0f) ? 1.0f : 0.0f;
    }
    *valid_a = va;
    return (label_at(2 * pair + 1, r, c)[3] == 1.0f ? 1.0f : 0.0f) * va;
  };

  double cnt = 0.0, lost = 0.0;
  for (long i = t; i < cells; i += LT) {
    Warp k;
    float va;
    cnt += mask_of(i, &k, &va);
    lost += va == 0.0f ? 1.0 : 0.0;
  }
  const float valid = (float)(block_sum(cnt, red) + 1.0);
  const double n_lost = block_sum(lost, red);

  double s_nll = 0.0, s_bad = 0.0;
  for (long i = t; i < cells; i += LT) {
    Warp k;
    float va;
    const float m = mask_of(i, &k, &va);
    const long pair = i / hw;
    const int rem = (int)(i - pair * hw);
    const int r = rem / p.w, c = rem - r * p.w;
    const float* l00 = label_at(2 * pair, k.iy0, k.ix0);
    const float* l01 = label_at(2 * pair, k.iy1, k.ix0);
    const float* l10 = label_at(2 * pair, k.iy0, k.ix1);
    const float* l11 = label_at(2 * pair, k.iy1, k.ix1);
    const float* gb = label_at(2 * pair + 1, r, c);
    const float w00 = k.wx0 * k.wy0, w01 = k.wx0 * k.wy1, w10 = k.wx1 * k.wy0, w11 = k.wx1 * k.wy1;
    float e[3], dpx[3], dpy[3];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      const float xm = ((w00 * l00[ch] + w01 * l01[ch]) + w10 * l10[ch]) + w11 * l11[ch];   // the sampler's add_n order
      e[ch] = xm - gb[ch];
      // the weights' derivatives: d wx0 / d px = -1, d wx1 / d px = +1, and the same in y
      dpx[ch] = k.wy0 * (l10[ch] - l00[ch]) + k.wy1 * (l11[ch] - l01[ch]);
      dpy[ch] = k.wx0 * (l01[ch] - l00[ch]) + k.wx1 * (l11[ch] - l10[ch]);
    }
    const float d = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2];
    const float st = p.sigma_trans[i];
    const float tv = st * st;
    const float sm = sqrtf(p.eps2 + fmaxf(tv, p.eps2));   // label a is certain: its variance is the floor
    const float u = fmaxf(sm, p.min_unc);
    const float iu2 = 1.0f / (u * u);
    float l = 3.0f * logf(u) + d * 0.5f * iu2;
    float live = m / valid;
    if (p.has_clip && l > p.clip) {      // tf.minimum(loss_map, clip): no gradient through the constant
      l = p.clip;
      live = 0.0f;
    }
    s_nll += (double)(m * l);
    s_bad += (m * d - p.thr2 > 0.0f) ? 1.0 : 0.0;
    const float gx = live * iu2;
    p.d_flow[2 * i] = gx * ((e[0] * dpx[0] + e[1] * dpx[1]) + e[2] * dpx[2]);
    p.d_flow[2 * i + 1] = gx * ((e[0] * dpy[0] + e[1] * dpy[1]) + e[2] * dpy[2]);
    p.d_sigma[i] = (sm > p.min_unc && tv > p.eps2) ? live * (3.0f / u - d * iu2 / u) * (st / sm) : 0.0f;
  }
  const double nll = block_sum(s_nll, red);
  const double bad = block_sum(s_bad, red);
  if (t == 0) {
    const double v = (double)valid;
    p.stats[0] = (float)(nll / v);
    p.stats[1] = (float)((v - bad) / v);
    p.stats[2] = valid;
    p.stats[3] = (float)n_lost;
    for (int k = 4; k < 16; ++k) p.stats[k] = 0.0f;
  }
}

inline bool aligned16(const void* a) { return (reinterpret_cast<uintptr_t>(a) & 15) == 0; }

}  // namespace

extern "C" int kfn_cost_volume_backward(const float* d_vol, float* d_f2, float* d_f1, int N, int H, int W, int C, void* stream) {
  KFN_REQUIRE(d_vol && d_f2 && d_f1, "kfn_cost_volume_backward: null argument");
  KFN_REQUIRE(N > 0 && H > 0 && W > 0 && C > 0 && C % 4 == 0, "kfn_cost_volume_backward: bad shape N=%d H=%d W=%d C=%d", N, H, W, C);
  KFN_REQUIRE(aligned16(d_vol) && aligned16(d_f2) && aligned16(d_f1), "kfn_cost_volume_backward: misaligned buffer");
  const long threads = 2L * N * H * W * (C / 4);
  const long blocks = (threads + 255) / 256;
  KFN_REQUIRE(blocks < (1L << 31), "kfn_cost_volume_backward: %dx%dx%dx%d is too large for one launch", N, H, W, C);
  hipLaunchKernelGGL(cost_volume_backward_kernel, dim3((unsigned)blocks), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                     reinterpret_cast<const f32x4*>(d_vol), reinterpret_cast<f32x4*>(d_f2), reinterpret_cast<f32x4*>(d_f1), N, H, W,
                     C / 4);
  KFN_LAUNCH_CHECK("cost_volume_backward_kernel");
  return KFN_OK;
}

extern "C" int kfn_flow_head_backward(const float* d_flow, const float* prob, const float* d_sigma, const float* sigma_trans,
                                      float* d_logits, int ld_logits, float* d_pre, int ld_pre, long N, void* stream) {
  KFN_REQUIRE(d_flow && prob && d_sigma && sigma_trans && d_logits && d_pre, "kfn_flow_head_backward: null argument");
  KFN_REQUIRE(N > 0 && (N + 3) / 4 < (1L << 31), "kfn_flow_head_backward: N = %ld", N);
  KFN_REQUIRE(ld_logits >= 4 && ld_logits % 4 == 0 && ld_pre >= 1 && ld_pre <= 64,
              "kfn_flow_head_backward: bad pixel strides (%d: a multiple of 4; %d: 1..64)", ld_logits, ld_pre);
  KFN_REQUIRE(aligned16(d_logits), "kfn_flow_head_backward: d_logits must be 16-byte aligned");
  hipLaunchKernelGGL(flow_head_backward_kernel, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                     d_flow, prob, d_sigma, sigma_trans, d_logits, ld_logits, d_pre, ld_pre, N);
  KFN_LAUNCH_CHECK("flow_head_backward_kernel");
  return KFN_OK;
}

extern "C" int kfn_l2norm_backward(const float* x, int ldx, const float* g, int ldg, float* dx, int ld_dx, long pixels, int C,
                                   void* stream) {
  KFN_REQUIRE(x && g && dx, "kfn_l2norm_backward: null argument");
  KFN_REQUIRE(C == 32, "kfn_l2norm_backward: C = %d, only feat7's 32 channels are built", C);
  KFN_REQUIRE(pixels > 0 && (pixels * 8 + 255) / 256 < (1L << 31), "kfn_l2norm_backward: pixels = %ld", pixels);
  KFN_REQUIRE(ldx >= C && ldg >= C && ld_dx >= C && ((ldx | ldg | ld_dx) & 3) == 0,
              "kfn_l2norm_backward: pixel strides (%d, %d, %d) must be multiples of 4 and at least %d", ldx, ldg, ld_dx, C);
  KFN_REQUIRE(aligned16(x) && aligned16(g) && aligned16(dx), "kfn_l2norm_backward: misaligned buffer");
  hipLaunchKernelGGL(l2norm_backward_kernel, dim3((unsigned)((pixels * 8 + 255) / 256)), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), x, ldx, g, ldg, dx, ld_dx, pixels);
  KFN_LAUNCH_CHECK("l2norm_backward_kernel");
  return KFN_OK;
}

extern "C" int kfn_flow_loss_grad(const kfn_flow_loss_desc* d, const float* flow_xy, const float* sigma_trans, const float* labels,
                                  float* d_flow, float* d_sigma, float* stats, void* stream) {
  KFN_REQUIRE(d && flow_xy && sigma_trans && labels && d_flow && d_sigma && stats, "kfn_flow_loss_grad: null argument");
  KFN_REQUIRE(d->struct_size == (int32_t)sizeof(kfn_flow_loss_desc), "kfn_flow_loss_grad: struct_size %d, expected %d",
              (int)d->struct_size, (int)sizeof(kfn_flow_loss_desc));
  KFN_REQUIRE(d->P > 0 && d->h > 1 && d->w > 1 && (long)d->P * d->h * d->w < (1L << 24), "kfn_flow_loss_grad: bad grid %dx%dx%d",
              d->P, d->h, d->w);
  KFN_REQUIRE(d->label_stride >= 1, "kfn_flow_loss_grad: bad label_stride %d", d->label_stride);
  KFN_REQUIRE(d->min_uncertainty > 0.0 && d->dist_threshold >= 0.0, "kfn_flow_loss_grad: bad thresholds");
  FlowLossArgs a;
  a.flow = flow_xy; a.sigma_trans = sigma_trans; a.labels = labels; a.d_flow = d_flow; a.d_sigma = d_sigma; a.stats = stats;
  a.P = d->P; a.h = d->h; a.w = d->w; a.label_stride = d->label_stride;
  a.has_clip = d->has_loss_clip; a.clip = d->loss_clip;
  // the reference squares the Python doubles and TensorFlow rounds each product once: 0x3B23D70A for 0.05
  a.thr2 = (float)(d->dist_threshold * d->dist_threshold);
  a.min_unc = (float)d->min_uncertainty;
  a.eps2 = (float)(d->min_uncertainty * d->min_uncertainty);
  hipLaunchKernelGGL(flow_loss_grad_kernel, dim3(1), dim3(LT), 0, reinterpret_cast<hipStream_t>(stream), a);
  KFN_LAUNCH_CHECK("flow_loss_grad_kernel");
  return KFN_OK;
}
