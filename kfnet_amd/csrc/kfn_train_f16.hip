// kfn_train_f16.hip -- mixed-precision training of SCoordNet's convolutions (gfx950): the weight gradient as a GEMM on
// v_mfma_f32_32x32x16_f16 (fp32 tensors in memory, operands rounded to IEEE halfs while staged, fp32 accumulation).  The fp32
// form, the reduction of the planes and the weight packs (float and half) are in kfn_train.hip; DESIGN.md 6h.
#include "kfn_train_shared.h"

namespace {

using kfn::WG_BM;
using kfn::WG_BP_F16;
using kfn::WgradArgs;
using kfn::WgradPlan;

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef short s16x4 __attribute__((__vector_size__(4 * sizeof(short))));
typedef short s16x8 __attribute__((__vector_size__(8 * sizeof(short))));

// ---------------------------------------------------------------------------------------------------------------------
// The GEMM of wgrad_mfma_kernel (kfn_train.hip) with fp16 operands: dW[k][co] = sum_p A[p][k] dZ[p][co], row Ktot of A the
// constant 1.  Same workgroup tile (128 k x 64*TN co, 4 waves, 2 x TN accumulators of 32x32 per wave), same runs of pixels,
// same workspace planes.  A stage is 32 pixels = two k-steps of v_mfma_f32_32x32x16_f16.
//
// The reduction index is the pixel, and the fp16 MFMA takes 8 consecutive k per lane (lane l: A[row l & 31][k = 8 (l >> 5)
// + j], B[k = 8 (l >> 5) + j][col l & 31], j = 0..7): 8 pixels of ONE channel, a column of the NHWC data.  The tiles are
// staged as they come, [pixel][channel] halfs (a float4 of four channels -> one 8-byte store), and read column-major with
// ds_read_b64_tr_b16: per 16 lanes it takes a block of 4 rows (pixels) x 16 columns (channels), lane 4q + c supplying the
// address of row q, columns 4c .. 4c + 3, and hands lane i column i of the four rows.  Two such reads (pixels 8h .. 8h + 3
// and 8h + 4 .. 8h + 7) make a fragment.  Every lane of the wave supplies an in-bounds address and EXEC is full: the loop
// bounds are uniform, short runs are padded with zero pixels, never masked.
//
// LDS rows are the tile width + 32 halfs (320 B for 128 channels, 192 B for 64): the four rows a 32-lane half reads, 64 B
// each, fall on the four quarters of the 256-byte bank row -- no conflicts.
// ---------------------------------------------------------------------------------------------------------------------
template <int TN>
__global__ __launch_bounds__(256, 2) void wgrad_f16_kernel(WgradArgs p) {
  constexpr int BP = WG_BP_F16;
  constexpr int BN = 64 * TN;
  constexpr int LDA = WG_BM + 32, LDB = BN + 32;   // halfs
  __shared__ __attribute__((aligned(16))) _Float16 As[BP * LDA];
  __shared__ __attribute__((aligned(16))) _Float16 Bs[BP * LDB];

  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int li = lane & 31, lh = lane >> 5;
  const int wm = wave >> 1, wn = wave & 1;
  const int tile_n = blockIdx.x % p.tiles_n, tile_m = blockIdx.x / p.tiles_n;
  const int m0 = tile_m * WG_BM, n0 = tile_n * BN;
  const long pbeg = (long)blockIdx.y * p.chunk;
  const long pend = (pbeg + p.chunk < p.P) ? pbeg + p.chunk : p.P;

  // A loader: float4 j of the 128-row tile, pixels apr + 8 i of the stage.  Its tap is fixed for the whole launch.
  constexpr int APASS = BP / 8;
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
  // B loader (Cout % 32 == 0, ldz % 4 == 0, dz 16-byte aligned: whole float4 only)
  constexpr int BJ = BN / 4;              // float4 per pixel row
  constexpr int BROWS = 256 / BJ;         // pixel rows covered per pass (8 for TN = 2, 16 for TN = 1)
  constexpr int BPASS = BP / BROWS;
  const int bj = t % BJ, bpr = t / BJ;
  const int bco = n0 + bj * 4;

  f32x16 acc[2][TN];
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int ni = 0; ni < TN; ++ni)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[mi][ni][e] = 0.f;

  float4 ra[APASS], rb[BPASS];
  const int HoWo = p.Ho * p.Wo;

  auto fetch = [&](long ps) {
#pragma unroll
    for (int i = 0; i < APASS; ++i) {
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
      if (pp < pend && bco < p.Cout) v = *reinterpret_cast<const float4*>(p.dz + pp * p.ldz + bco);
      rb[i] = v;
    }
  };
  auto halfs = [](const float4& v) {   // round to nearest even, once
    const f16x4 h = {(_Float16)v.x, (_Float16)v.y, (_Float16)v.z, (_Float16)v.w};
    return h;
  };

  // transposed-read addresses: group g = lane >> 4 takes columns 16 (g & 1) .. + 15 of pixels 8 (g >> 1) .. + 7
  const int tq = (lane >> 2) & 3, tc = lane & 3;
  const int t_row = 8 * lh + tq, t_col = 16 * ((lane >> 4) & 1) + 4 * tc;
  auto frag = [&](const _Float16* tile, int ld, int ks, int col0) {
    typedef __attribute__((address_space(3))) s16x4 lds_s16x4;
    const _Float16* a0 = tile + (16 * ks + t_row) * ld + col0 + t_col;
    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(a0));
    const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(a0 + 4 * ld));
    const s16x8 f = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
    return __builtin_bit_cast(f16x8, f);
  };

  if (pbeg < pend) fetch(pbeg);
  for (long ps = pbeg; ps < pend; ps += BP) {
    __syncthreads();   // the previous stage's fragment reads are done
#pragma unroll
    for (int i = 0; i < APASS; ++i) *reinterpret_cast<f16x4*>(&As[(apr + 8 * i) * LDA + aj * 4]) = halfs(ra[i]);
#pragma unroll
    for (int i = 0; i < BPASS; ++i) *reinterpret_cast<f16x4*>(&Bs[(bpr + BROWS * i) * LDB + bj * 4]) = halfs(rb[i]);
    __syncthreads();
    if (ps + BP < pend) fetch(ps + BP);
#pragma unroll
    for (int ks = 0; ks < BP / 16; ++ks) {
      f16x8 a[2], b[TN];
#pragma unroll
      for (int mi = 0; mi < 2; ++mi) a[mi] = frag(As, LDA, ks, (wm * 2 + mi) * 32);
#pragma unroll
      for (int ni = 0; ni < TN; ++ni) b[ni] = frag(Bs, LDB, ks, (wn * TN + ni) * 32);
#pragma unroll
      for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int ni = 0; ni < TN; ++ni)
          acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[mi], b[ni], acc[mi][ni], 0, 0, 0);
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

}  // namespace

int kfn::wgrad_f16_launch(const WgradArgs& a, const WgradPlan& pl, hipStream_t s) {
  const dim3 grid((unsigned)(pl.tiles_m * pl.tiles_n), (unsigned)pl.splits);
  if (pl.tn == 1) hipLaunchKernelGGL(wgrad_f16_kernel<1>, grid, dim3(256), 0, s, a);
  else hipLaunchKernelGGL(wgrad_f16_kernel<2>, grid, dim3(256), 0, s, a);
  KFN_LAUNCH_CHECK("wgrad_f16_kernel");
  return KFN_OK;
}
