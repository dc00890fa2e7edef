// kfn_train.hip -- the backward pass of SCoordNet's convolutions (gfx950): weight gradients as an fp32 MFMA GEMM whose
// reduction dimension is the pixels, conv1a's weight gradient from the uint8 frame, the ReLU gradient, and the device-side
// weight packs of the forward and input-gradient launches.  Replaces what tf.gradients derives from tf.layers.conv2d
// (cnn_wrapper/network.py:116-135) under AdamOptimizer.minimize (KFNet/train.py:313-314).  DESIGN.md "Training".
//
// Input gradients are NOT here: they run on the forward kernels (kfn_conv2d_nhwc) with the packs made below.  The fp16-operand
// weight gradient is in kfn_train_f16.hip; kfn_train_shared.h holds what the two files share.
#include "kfn_train_shared.h"

namespace {

using kfn::WG_BM;
using kfn::WG_BP;
using kfn::WgradArgs;
using kfn::WgradPlan;

typedef float f32x16 __attribute__((ext_vector_type(16)));

// ---------------------------------------------------------------------------------------------------------------------
// dW[k][co] = sum_p A[p][k] dZ[p][co], k = (kh, kw, ci) flattened (TF HWIO), p = (n, oy, ox) the forward conv's OUTPUT
// pixels, A[p][k] = X[n, oy*s + kh - pad_t, ox*s + kw - pad_l, ci] (0 outside).  Row k = Ktot of A is the constant 1, so
// the same GEMM yields db[co] = sum_p dZ[p][co].
//
// Workgroup = 4 waves = a 128 (k) x 64*TN (co) tile of the result, held in 2 x TN accumulators of 32x32 per wave, over one
// contiguous run of pixels (split `blockIdx.y`).  A stage = 16 pixels: every thread fetches two float4 of A and two (one
// for TN = 1) of dZ into registers while the MFMAs of the previous stage run, then the tile goes through one LDS buffer.
// v_mfma_f32_32x32x2_f32 takes A[i = lane & 31][k = lane >> 5] and B[k = lane >> 5][j = lane & 31]: with the pixel as k,
// a lane's operands are single LDS words at [pixel][channel], the natural NHWC order -- no transpose anywhere.
// Every split writes its partial tile into its own plane of the workspace; wgrad_reduce_kernel adds the planes in the
// order 0 .. splits-1.  No atomics: the result is a fixed function of the shapes.
// ---------------------------------------------------------------------------------------------------------------------
constexpr int WG_TARGET = 1024;   // workgroups a launch aims for (4 per CU of an MI355X); a constant, so that the split --
                                  // and with it the summation order -- depends on the shapes alone, not on the device
constexpr int WG_MIN_CHUNK = 512; // fewest pixels per split

template <int TN>
__global__ __launch_bounds__(256, 2) void wgrad_mfma_kernel(WgradArgs p) {
  constexpr int BN = 64 * TN;
  constexpr int LDA = WG_BM + 32, LDB = BN + 32;    // row r+1 starts 32 banks after row r: the two half-waves of a fragment
                                                    // read (pixels 2t and 2t+1) never share a bank
  __shared__ __attribute__((aligned(16))) float As[WG_BP * LDA];
  __shared__ __attribute__((aligned(16))) float Bs[WG_BP * LDB];

  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int li = lane & 31, lh = lane >> 5;
  const int wm = wave >> 1, wn = wave & 1;
  const int tile_n = blockIdx.x % p.tiles_n, tile_m = blockIdx.x / p.tiles_n;
  const int m0 = tile_m * WG_BM, n0 = tile_n * BN;
  const long pbeg = (long)blockIdx.y * p.chunk;
  const long pend = (pbeg + p.chunk < p.P) ? pbeg + p.chunk : p.P;

  // A loader: float4 j of the 128-row tile, pixels pr and pr + 8 of the stage.  Its tap is fixed for the whole launch.
  const int aj = t & 31, apr = t >> 5;
  const int kbase = m0 + aj * 4;
  int a_kind;   // 0 = zero rows, 1 = input tap, 2 = the bias row (1, 0, 0, 0)
  int a_dy = 0, a_dx = 0, a_ci = 0;
  if (kbase < p.Ktot) {
    const int tap = kbase / p.Cin;
    a_ci = kbase - tap * p.Cin;
    a_dy = tap / p.kw - p.pad_t;
    a_dx = tap % p.kw - p.pad_l;
    a_kind = 1;
  } else {
    a_kind = (kbase == p.Ktot) ? 2 : 0;
  }
  // B loader
  constexpr int BJ = BN / 4;              // float4 per pixel row
  constexpr int BROWS = 256 / BJ;         // pixel rows covered per pass (8 for TN = 2, 16 for TN = 1)
  constexpr int BPASS = WG_BP / BROWS;
  const int bj = t % BJ, bpr = t / BJ;
  const int bco = n0 + bj * 4;

  f32x16 acc[2][TN];
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int ni = 0; ni < TN; ++ni)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[mi][ni][e] = 0.f;

  float4 ra[2], rb[BPASS];
  const int HoWo = p.Ho * p.Wo;

  auto fetch = [&](long ps) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const long pp = ps + apr + 8 * i;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (pp < pend && a_kind != 0) {
        if (a_kind == 2) {
          v.x = 1.f;
        } else {
          const int n = (int)(pp / HoWo);
          const int rem = (int)(pp - (long)n * HoWo);
          const int oy = rem / p.Wo, ox = rem - oy * p.Wo;
          const int iy = oy * p.stride + a_dy, ix = ox * p.stride + a_dx;
          if ((unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)p.W)
            v = *reinterpret_cast<const float4*>(p.x + (((long)n * p.H + iy) * p.W + ix) * p.ldx + a_ci);
        }
      }
      ra[i] = v;
    }
#pragma unroll
    for (int i = 0; i < BPASS; ++i) {
      const long pp = ps + bpr + BROWS * i;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (pp < pend && bco < p.Cout) {
        const float* src = p.dz + pp * p.ldz + bco;
        if (p.vec_b && bco + 3 < p.Cout) {
          v = *reinterpret_cast<const float4*>(src);
        } else {
          v.x = src[0];
          if (bco + 1 < p.Cout) v.y = src[1];
          if (bco + 2 < p.Cout) v.z = src[2];
          if (bco + 3 < p.Cout) v.w = src[3];
        }
      }
      rb[i] = v;
    }
  };

  if (pbeg < pend) fetch(pbeg);
  for (long ps = pbeg; ps < pend; ps += WG_BP) {
    __syncthreads();   // the previous stage's fragment reads are done
#pragma unroll
    for (int i = 0; i < 2; ++i) *reinterpret_cast<float4*>(&As[(apr + 8 * i) * LDA + aj * 4]) = ra[i];
#pragma unroll
    for (int i = 0; i < BPASS; ++i) *reinterpret_cast<float4*>(&Bs[(bpr + BROWS * i) * LDB + bj * 4]) = rb[i];
    __syncthreads();
    if (ps + WG_BP < pend) fetch(ps + WG_BP);
#pragma unroll
    for (int kk = 0; kk < WG_BP / 2; ++kk) {
      float a[2], b[TN];
#pragma unroll
      for (int mi = 0; mi < 2; ++mi) a[mi] = As[(2 * kk + lh) * LDA + (wm * 2 + mi) * 32 + li];
#pragma unroll
      for (int ni = 0; ni < TN; ++ni) b[ni] = Bs[(2 * kk + lh) * LDB + (wn * TN + ni) * 32 + li];
#pragma unroll
      for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int ni = 0; ni < TN; ++ni)
          acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[mi], b[ni], acc[mi][ni], 0, 0, 0);
    }
  }

  // C/D layout of the 32x32 MFMA: col = lane & 31, row = (e & 3) + 8*(e >> 2) + 4*(lane >> 5)
  float* plane = p.ws + (long)blockIdx.y * (p.Ktot + 1) * p.Cout;
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int ni = 0; ni < TN; ++ni) {
      const int col = n0 + (wn * TN + ni) * 32 + li;
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int row = m0 + (wm * 2 + mi) * 32 + (e & 3) + 8 * (e >> 2) + 4 * lh;
        if (row <= p.Ktot && col < p.Cout) plane[(long)row * p.Cout + col] = acc[mi][ni][e];
      }
    }
}

// dw[k][co] = sum_s ws[s][k][co], s ascending; the last row of a plane goes to db
__global__ __launch_bounds__(256) void wgrad_reduce_kernel(const float* __restrict__ ws, int splits, long rows_w, int Cout,
                                                           float* __restrict__ dw, float* __restrict__ db) {
  const long n_w = rows_w * Cout, n = n_w + Cout;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    float s = ws[i];
    for (int k = 1; k < splits; ++k) s += ws[(long)k * n + i];
    if (i < n_w) dw[i] = s;
    else if (db) db[i - n_w] = s;
  }
}

int wgrad_plan(const kfn_conv_desc* d, WgradPlan* pl, const char* who) {
  KFN_REQUIRE(d->N > 0 && d->H > 0 && d->W > 0, "%s: bad shape %dx%dx%d", who, d->N, d->H, d->W);
  KFN_REQUIRE(d->Cin > 0 && d->Cin % 16 == 0, "%s: Cin=%d must be a multiple of 16", who, d->Cin);
  KFN_REQUIRE(d->ldx >= d->Cin && d->ldx % 4 == 0, "%s: bad ldx=%d", who, d->ldx);
  KFN_REQUIRE(d->Cout > 0 && d->ldy >= d->Cout, "%s: bad Cout=%d ldy=%d (ldy is dZ's pixel stride)", who, d->Cout, d->ldy);
  KFN_REQUIRE((d->kh == 3 && d->kw == 3) || (d->kh == 1 && d->kw == 1), "%s: kernel %dx%d (3x3 and 1x1 only)", who, d->kh, d->kw);
  KFN_REQUIRE(d->stride == 1 || d->stride == 2, "%s: stride %d unsupported", who, d->stride);
  KFN_REQUIRE(!d->transposed, "%s: the descriptor is the FORWARD convolution's (transposed = 0)", who);
  KFN_REQUIRE(d->operand_dtype == KFN_OPERAND_F32 || d->operand_dtype == KFN_OPERAND_F16, "%s: operand_dtype %d (fp32 or fp16 operands)",
              who, d->operand_dtype);
  KFN_REQUIRE(d->x_dtype == KFN_ACT_F32 && d->y_dtype == KFN_ACT_F32, "%s: fp32 activations in memory only", who);
  const bool f16 = d->operand_dtype == KFN_OPERAND_F16;
  // the fp16 kernel stages whole float4 of dZ and 32-column MFMA tiles: nothing ragged in the channels
  KFN_REQUIRE(!f16 || (d->Cin % 32 == 0 && d->Cout % 32 == 0), "%s: fp16 operands need Cin %% 32 == 0 and Cout %% 32 == 0 (Cin=%d, Cout=%d)",
              who, d->Cin, d->Cout);
  KFN_REQUIRE(!f16 || d->ldy % 4 == 0, "%s: fp16 operands need dZ's pixel stride ldy %% 4 == 0 (ldy=%d)", who, d->ldy);
  kfn::same_pad(d->H, d->kh, d->stride, &pl->Ho, &pl->pad_t);
  kfn::same_pad(d->W, d->kw, d->stride, &pl->Wo, &pl->pad_l);
  pl->Ktot = d->kh * d->kw * d->Cin;
  pl->P = (long)d->N * pl->Ho * pl->Wo;
  KFN_REQUIRE((long)d->N * d->H * d->W * d->ldx < (1L << 40) && pl->P < (1L << 31), "%s: tensor too large", who);
  pl->tn = d->Cout <= 64 ? 1 : 2;
  pl->tiles_m = kfn::ceil_div(pl->Ktot + 1, WG_BM);
  pl->tiles_n = kfn::ceil_div(d->Cout, 64 * pl->tn);
  long splits = WG_TARGET / ((long)pl->tiles_m * pl->tiles_n);
  const long most = pl->P / WG_MIN_CHUNK;
  if (splits > most) splits = most;
  if (splits < 1) splits = 1;
  long chunk = (pl->P + splits - 1) / splits;
  const int stage = f16 ? kfn::WG_BP_F16 : WG_BP;
  chunk = (chunk + stage - 1) / stage * stage;
  pl->chunk = chunk;
  pl->splits = (int)((pl->P + chunk - 1) / chunk);
  KFN_REQUIRE(pl->splits <= 65535, "%s: too many splits", who);
  return KFN_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// conv1a: dW[27][C] and db[C] from the uint8 frame.  The layer has 3 input channels, far below an MFMA tile, and 28 x C
// results: one workgroup walks FC_CHUNK pixels, stages the 27 preprocessed taps (+ the constant 1) of 64 pixels at a time
// in LDS, and every thread keeps up to 7 of the 28*C sums (C <= 64).  Partial sums per workgroup, reduced as above.
// ---------------------------------------------------------------------------------------------------------------------
constexpr int FC_CHUNK = 2048;
constexpr int FC_SUB = 64;

__global__ __launch_bounds__(256) void first_wgrad_kernel(const uint8_t* __restrict__ img, const float* __restrict__ dz,
                                                          float* __restrict__ ws, int H, int W, long P, int C) {
  __shared__ float taps[FC_SUB][28];
  const int t = threadIdx.x;
  const long pbeg = (long)blockIdx.x * FC_CHUNK;
  const long pend = (pbeg + FC_CHUNK < P) ? pbeg + FC_CHUNK : P;
  const int n_out = 28 * C;
  float acc[7];
  int kk[7], cc[7];
#pragma unroll
  for (int i = 0; i < 7; ++i) {
    acc[i] = 0.f;
    const int idx = t + 256 * i;
    kk[i] = idx < n_out ? idx / C : -1;
    cc[i] = idx < n_out ? idx % C : 0;
  }
  for (long ps = pbeg; ps < pend; ps += FC_SUB) {
    __syncthreads();
    for (int id = t; id < FC_SUB * 28; id += 256) {
      const int px = id / 28, k = id - px * 28;
      const long pp = ps + px;
      float v = 0.f;
      if (pp < pend) {
        if (k == 27) {
          v = 1.f;
        } else {
          const int tap = k / 3, ci = k - tap * 3;
          const long n = pp / ((long)H * W);
          const int rem = (int)(pp - n * H * W);
          const int y = rem / W + tap / 3 - 1, x = rem % W + tap % 3 - 1;
          if ((unsigned)y < (unsigned)H && (unsigned)x < (unsigned)W)
            v = ((float)img[((n * H + y) * W + x) * 3 + ci] - 128.0f) * 0.00625f;   // SCoordNet.preprocess, as kfn_first_conv_u8
        }
      }
      taps[px][k] = v;
    }
    __syncthreads();
    const int cnt = (int)((pend - ps < FC_SUB) ? pend - ps : FC_SUB);
    for (int px = 0; px < cnt; ++px) {
      const float* g = dz + (ps + px) * C;
#pragma unroll
      for (int i = 0; i < 7; ++i)
        if (kk[i] >= 0) acc[i] = fmaf(taps[px][kk[i]], g[cc[i]], acc[i]);
    }
  }
  float* plane = ws + (long)blockIdx.x * n_out;
#pragma unroll
  for (int i = 0; i < 7; ++i)
    if (kk[i] >= 0) plane[t + 256 * i] = acc[i];
}

__global__ __launch_bounds__(256) void relu_grad_kernel(const float* __restrict__ y, int ldy, float* __restrict__ dz, int ldz,
                                                        long P, int C) {
  const long n = P * C;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const long px = i / C;
    const int c = (int)(i - px * C);
    if (!(y[px * ldy + c] > 0.f)) dz[px * ldz + c] = 0.f;
  }
}

// out[r][(a, b, c)], r < rows_pad, c < cols_pad: the matrix kfn_conv2d_nhwc multiplies by (K contiguous per output channel);
// T = float, or _Float16 for the fp16-operand launches (the value rounded once, to nearest even)
template <typename T>
__global__ __launch_bounds__(256) void pack_weights_kernel(const float* __restrict__ w, int kh, int kw, int Cin, int Cout,
                                                           int kind, int rows_pad, int cols_pad, T* __restrict__ out) {
  const long n = (long)rows_pad * kh * kw * cols_pad;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const int c = (int)(i % cols_pad);
    long q = i / cols_pad;
    const int b = (int)(q % kw);
    q /= kw;
    const int a = (int)(q % kh);
    const int r = (int)(q / kh);
    float v = 0.f;
    if (kind == KFN_PACK_FORWARD) {
      if (r < Cout && c < Cin) v = w[(((long)a * kw + b) * Cin + c) * Cout + r];
    } else if (kind == KFN_PACK_INPUT_GRAD_S1) {
      if (r < Cin && c < Cout) v = w[(((long)(kh - 1 - a) * kw + (kw - 1 - b)) * Cin + r) * Cout + c];
    } else {
      if (r < Cin && c < Cout) v = w[(((long)a * kw + b) * Cin + r) * Cout + c];
    }
    out[i] = (T)v;
  }
}

int pack_dims(int kh, int kw, int Cin, int Cout, int kind, int* rows_pad, int* cols_pad) {
  KFN_REQUIRE(kh > 0 && kw > 0 && kh * kw <= 32 && Cin > 0 && Cout > 0, "kfn_pack_conv_weights: bad kernel shape %dx%dx%dx%d",
              kh, kw, Cin, Cout);
  KFN_REQUIRE(kind == KFN_PACK_FORWARD || kind == KFN_PACK_INPUT_GRAD_S1 || kind == KFN_PACK_INPUT_GRAD_S2,
              "kfn_pack_conv_weights: unknown kind %d", kind);
  // The input gradient is the SAME convolution of dz with the rotated kernel only when SAME pads both sides alike.  An even
  // kernel pads (k - 1) / 2 in front and one more behind, the rotated one needs the larger share in front: kfn_conv2d_nhwc
  // on such a pack would return the gradient shifted by one pixel.
  KFN_REQUIRE(kind != KFN_PACK_INPUT_GRAD_S1 || (kh % 2 == 1 && kw % 2 == 1),
              "kfn_pack_conv_weights: KFN_PACK_INPUT_GRAD_S1 needs an odd kernel (%dx%d): SAME padding of an even kernel is "
              "asymmetric, so the stride-1 convolution of dz with the rotated kernel is the input gradient shifted by one pixel",
              kh, kw);
  const int rows = kind == KFN_PACK_FORWARD ? Cout : Cin, cols = kind == KFN_PACK_FORWARD ? Cin : Cout;
  *rows_pad = (rows + 31) / 32 * 32;
  *cols_pad = (cols + 15) / 16 * 16;
  return KFN_OK;
}

unsigned grid_for(long n) {
  long b = (n + 255) / 256;
  return (unsigned)(b < 1 ? 1 : (b > 8192 ? 8192 : b));
}

}  // namespace

extern "C" int kfn_conv2d_grad_weights_workspace_bytes(const kfn_conv_desc* d, size_t* bytes) {
  KFN_REQUIRE(d && bytes, "kfn_conv2d_grad_weights_workspace_bytes: null argument");
  KFN_CONV_DESC_IN(d, "kfn_conv2d_grad_weights_workspace_bytes");
  WgradPlan pl;
  int rc = wgrad_plan(d, &pl, "kfn_conv2d_grad_weights_workspace_bytes");
  if (rc != KFN_OK) return rc;
  *bytes = (size_t)pl.splits * (pl.Ktot + 1) * d->Cout * sizeof(float);
  return KFN_OK;
}

// What kfn_conv2d_grad_weights will launch for `d`: wgrad_plan is the one function that decides, for the launcher, for the
// workspace size and for this report.  No device access.
extern "C" int kfn_conv2d_grad_weights_plan(const kfn_conv_desc* d, int* tn, int* tiles_m, int* tiles_n, int* splits, long* chunk) {
  KFN_REQUIRE(d && tn && tiles_m && tiles_n && splits && chunk, "kfn_conv2d_grad_weights_plan: null argument");
  KFN_CONV_DESC_IN(d, "kfn_conv2d_grad_weights_plan");
  WgradPlan pl;
  int rc = wgrad_plan(d, &pl, "kfn_conv2d_grad_weights_plan");
  if (rc != KFN_OK) return rc;
  *tn = pl.tn;
  *tiles_m = pl.tiles_m;
  *tiles_n = pl.tiles_n;
  *splits = pl.splits;
  *chunk = pl.chunk;
  return KFN_OK;
}

extern "C" int kfn_conv2d_grad_weights(const kfn_conv_desc* d, const float* x, const float* dz, float* dw, float* db,
                                       float* workspace, void* stream) {
  KFN_REQUIRE(d && x && dz && dw && workspace, "kfn_conv2d_grad_weights: null argument");
  KFN_CONV_DESC_IN(d, "kfn_conv2d_grad_weights");
  WgradPlan pl;
  int rc = wgrad_plan(d, &pl, "kfn_conv2d_grad_weights");
  if (rc != KFN_OK) return rc;
  KFN_REQUIRE((reinterpret_cast<uintptr_t>(x) & 15) == 0 && ((reinterpret_cast<uintptr_t>(dz) | reinterpret_cast<uintptr_t>(dw) |
               reinterpret_cast<uintptr_t>(workspace)) & 3) == 0, "kfn_conv2d_grad_weights: x must be 16-byte aligned");
  WgradArgs a;
  a.x = x; a.dz = dz; a.ws = workspace;
  a.H = d->H; a.W = d->W; a.Cin = d->Cin; a.ldx = d->ldx; a.Cout = d->Cout; a.ldz = d->ldy;
  a.kw = d->kw; a.stride = d->stride; a.Ho = pl.Ho; a.Wo = pl.Wo; a.pad_t = pl.pad_t; a.pad_l = pl.pad_l;
  a.Ktot = pl.Ktot; a.P = pl.P; a.chunk = pl.chunk; a.tiles_n = pl.tiles_n;
  a.vec_b = (d->ldy % 4 == 0 && (reinterpret_cast<uintptr_t>(dz) & 15) == 0) ? 1 : 0;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (d->operand_dtype == KFN_OPERAND_F16) {
    KFN_REQUIRE(a.vec_b, "kfn_conv2d_grad_weights: fp16 operands need a 16-byte aligned dz");
    rc = kfn::wgrad_f16_launch(a, pl, s);
    if (rc != KFN_OK) return rc;
  } else {
    const dim3 grid((unsigned)(pl.tiles_m * pl.tiles_n), (unsigned)pl.splits);
    if (pl.tn == 1) hipLaunchKernelGGL(wgrad_mfma_kernel<1>, grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL(wgrad_mfma_kernel<2>, grid, dim3(256), 0, s, a);
    KFN_LAUNCH_CHECK("wgrad_mfma_kernel");
  }
  const long n = (long)(pl.Ktot + 1) * d->Cout;
  hipLaunchKernelGGL(wgrad_reduce_kernel, dim3(grid_for(n)), dim3(256), 0, s, workspace, pl.splits, (long)pl.Ktot, d->Cout, dw, db);
  KFN_LAUNCH_CHECK("wgrad_reduce_kernel");
  return KFN_OK;
}

namespace {
int first_wgrad_check(int N, int H, int W, int C1, const char* who) {
  KFN_REQUIRE(N > 0 && H > 0 && W > 0 && (long)N * H * W < (1L << 31), "%s: bad shape %dx%dx%d", who, N, H, W);
  KFN_REQUIRE(C1 > 0 && C1 % 16 == 0 && C1 <= 64, "%s: C1=%d must be 16, 32, 48 or 64", who, C1);
  return KFN_OK;
}
}  // namespace

extern "C" int kfn_first_conv_u8_grad_weights_workspace_bytes(int N, int H, int W, int C1, size_t* bytes) {
  KFN_REQUIRE(bytes, "kfn_first_conv_u8_grad_weights_workspace_bytes: null argument");
  int rc = first_wgrad_check(N, H, W, C1, "kfn_first_conv_u8_grad_weights_workspace_bytes");
  if (rc != KFN_OK) return rc;
  const long P = (long)N * H * W;
  *bytes = (size_t)((P + FC_CHUNK - 1) / FC_CHUNK) * 28 * C1 * sizeof(float);
  return KFN_OK;
}

extern "C" int kfn_first_conv_u8_grad_weights(const uint8_t* img, int N, int H, int W, const float* dz, int C1, float* dw,
                                              float* db, float* workspace, void* stream) {
  KFN_REQUIRE(img && dz && dw && workspace, "kfn_first_conv_u8_grad_weights: null argument");
  int rc = first_wgrad_check(N, H, W, C1, "kfn_first_conv_u8_grad_weights");
  if (rc != KFN_OK) return rc;
  const long P = (long)N * H * W;
  const int blocks = (int)((P + FC_CHUNK - 1) / FC_CHUNK);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(first_wgrad_kernel, dim3(blocks), dim3(256), 0, s, img, dz, workspace, H, W, P, C1);
  KFN_LAUNCH_CHECK("first_wgrad_kernel");
  hipLaunchKernelGGL(wgrad_reduce_kernel, dim3(grid_for(28L * C1)), dim3(256), 0, s, workspace, blocks, 27L, C1, dw, db);
  KFN_LAUNCH_CHECK("wgrad_reduce_kernel");
  return KFN_OK;
}

extern "C" int kfn_relu_grad(const float* y, int ldy, float* dz, int ldz, long P, int C, void* stream) {
  KFN_REQUIRE(y && dz, "kfn_relu_grad: null argument");
  KFN_REQUIRE(P > 0 && C > 0 && ldy >= C && ldz >= C, "kfn_relu_grad: bad shape P=%ld C=%d ldy=%d ldz=%d", P, C, ldy, ldz);
  hipLaunchKernelGGL(relu_grad_kernel, dim3(grid_for(P * C)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), y, ldy, dz,
                     ldz, P, C);
  KFN_LAUNCH_CHECK("relu_grad_kernel");
  return KFN_OK;
}

extern "C" int kfn_pack_conv_weights_floats(int kh, int kw, int Cin, int Cout, int kind, size_t* floats) {
  KFN_REQUIRE(floats, "kfn_pack_conv_weights_floats: null argument");
  int rp, cp;
  int rc = pack_dims(kh, kw, Cin, Cout, kind, &rp, &cp);
  if (rc != KFN_OK) return rc;
  *floats = (size_t)rp * kh * kw * cp;
  return KFN_OK;
}

extern "C" int kfn_pack_conv_weights(const float* w_hwio, int kh, int kw, int Cin, int Cout, int kind, float* out,
                                     void* stream) {
  KFN_REQUIRE(w_hwio && out, "kfn_pack_conv_weights: null argument");
  int rp, cp;
  int rc = pack_dims(kh, kw, Cin, Cout, kind, &rp, &cp);
  if (rc != KFN_OK) return rc;
  const long n = (long)rp * kh * kw * cp;
  hipLaunchKernelGGL(pack_weights_kernel<float>, dim3(grid_for(n)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), w_hwio,
                     kh, kw, Cin, Cout, kind, rp, cp, out);
  KFN_LAUNCH_CHECK("pack_weights_kernel");
  return KFN_OK;
}

extern "C" int kfn_pack_conv_weights_f16(const float* w_hwio, int kh, int kw, int Cin, int Cout, int kind, void* out_halfs,
                                         void* stream) {
  KFN_REQUIRE(w_hwio && out_halfs, "kfn_pack_conv_weights_f16: null argument");
  int rp, cp;
  int rc = pack_dims(kh, kw, Cin, Cout, kind, &rp, &cp);
  if (rc != KFN_OK) return rc;
  const long n = (long)rp * kh * kw * cp;
  hipLaunchKernelGGL(pack_weights_kernel<_Float16>, dim3(grid_for(n)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), w_hwio,
                     kh, kw, Cin, Cout, kind, rp, cp, reinterpret_cast<_Float16*>(out_halfs));
  KFN_LAUNCH_CHECK("pack_weights_kernel<_Float16>");
  return KFN_OK;
}
