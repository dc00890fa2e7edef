// kfn_labels.hip -- training labels from depth maps and camera poses (gfx950).
// Compiled with -ffp-contract=off: every operation below is one rounded fp32 operation of DESIGN.md 6d, in that order, so a
// numpy float32 restatement (tests/labels_ref.py) gives the same bits.  No division and no transcendental: every derived
// constant arrives as a float the host has rounded once (kfnet_amd.labels.DepthCamera.descriptor).
//   kfn_depth_labels   depth [B,H,W] uint16 + poses [B][12] -> (world x, y, z, mask) at colour pixels (s c, s r), s = 1 or 8:
//                      optional registration gather, validity window, back-projection, camera-to-world.
//   kfn_label_moments  per frame the ten fp64 sums n, sum d, upper triangle of sum d d^T of d = p - pivot over mask == 1:
//                      what the decorrelating transform (transform.txt) is computed from.
#include "kfn_common.h"

namespace {

constexpr int ST = 256;     // threads of a workgroup, both kernels
constexpr int PX = 8;       // adjacent pixels per thread at stride 1: one 16-byte depth load, eight 16-byte stores

typedef __attribute__((ext_vector_type(4))) unsigned u32x4;

struct LabelArgs {
  const uint16_t* depth;
  const float* poses;
  float* out;
  int B, H, W, s, ld, vec, reg;
  int raw_min, raw_max;
  float u, v, inv_fx, inv_fy, kx, ky, ud, vd, scale;
};

// the depth sample of colour pixel (x, y) under registration, or -1 when it leaves the depth image
__device__ __forceinline__ int registered(const LabelArgs& p, const uint16_t* frame, int x, int y) {
  const float xd = roundf(((float)x - p.u) * p.kx + p.ud);      // half away from zero
  const float yd = roundf(((float)y - p.v) * p.ky + p.vd);
  if (!(xd >= 0.0f && xd <= (float)(p.W - 1) && yd >= 0.0f && yd <= (float)(p.H - 1))) return -1;
  return (int)frame[(long)(int)yd * p.W + (int)xd];
}

__device__ __forceinline__ float4 label_of(const LabelArgs& p, const float* P, int x, int y, int raw) {
  if (raw < p.raw_min || raw > p.raw_max) return make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  const float z = (float)raw * p.scale;
  const float X = (((float)x - p.u) * p.inv_fx) * z;
  const float Y = (((float)y - p.v) * p.inv_fy) * z;
  float4 o;
  o.x = ((P[0] * X + P[1] * Y) + P[2] * z) + P[3];
  o.y = ((P[4] * X + P[5] * Y) + P[6] * z) + P[7];
  o.z = ((P[8] * X + P[9] * Y) + P[10] * z) + P[11];
  o.w = 1.0f;
  return o;
}

__device__ __forceinline__ void store_label(const LabelArgs& p, long pixel, float4 o) {
  float* dst = p.out + pixel * p.ld;
  if (p.vec) {
    *reinterpret_cast<float4*>(dst) = o;
  } else {
    dst[0] = o.x; dst[1] = o.y; dst[2] = o.z; dst[3] = o.w;
  }
}

// stride 1: PX adjacent pixels of one row per thread
__global__ __launch_bounds__(ST) void depth_labels_full_kernel(LabelArgs p) {
  const int groups = p.W / PX;
  const long total = (long)p.B * p.H * groups;
  const long id = (long)blockIdx.x * ST + threadIdx.x;
  if (id >= total) return;
  const int g = (int)(id % groups);
  const long row = id / groups;
  const int y = (int)(row % p.H), b = (int)(row / p.H);
  const uint16_t* frame = p.depth + (long)b * p.H * p.W;
  float P[12];
  for (int k = 0; k < 12; ++k) P[k] = p.poses[b * 12 + k];
  int raw[PX];
  if (p.reg) {
    for (int k = 0; k < PX; ++k) raw[k] = registered(p, frame, g * PX + k, y);
  } else {
    const u32x4 d = *reinterpret_cast<const u32x4*>(frame + (long)y * p.W + g * PX);
    raw[0] = (int)(d.x & 0xFFFFu); raw[1] = (int)(d.x >> 16);
    raw[2] = (int)(d.y & 0xFFFFu); raw[3] = (int)(d.y >> 16);
    raw[4] = (int)(d.z & 0xFFFFu); raw[5] = (int)(d.z >> 16);
    raw[6] = (int)(d.w & 0xFFFFu); raw[7] = (int)(d.w >> 16);
  }
  const long first = row * p.W + (long)g * PX;
  for (int k = 0; k < PX; ++k) store_label(p, first + k, label_of(p, P, g * PX + k, y, raw[k]));
}

// stride 8: one thread per output pixel (r, c) = colour pixel (8 c, 8 r)
__global__ __launch_bounds__(ST) void depth_labels_grid_kernel(LabelArgs p) {
  const int h = p.H / p.s, w = p.W / p.s;
  const long total = (long)p.B * h * w;
  const long id = (long)blockIdx.x * ST + threadIdx.x;
  if (id >= total) return;
  const int c = (int)(id % w);
  const long rest = id / w;
  const int r = (int)(rest % h), b = (int)(rest / h);
  const int x = c * p.s, y = r * p.s;
  const uint16_t* frame = p.depth + (long)b * p.H * p.W;
  float P[12];
  for (int k = 0; k < 12; ++k) P[k] = p.poses[b * 12 + k];
  const int raw = p.reg ? registered(p, frame, x, y) : (int)frame[(long)y * p.W + x];
  store_label(p, id, label_of(p, P, x, y, raw));
}

// ---- moments -----------------------------------------------------------------------------------------------------------
// One workgroup per frame: thread t adds pixels t, t + ST, ... in that order, then a fixed LDS tree joins the ST partial
// sums.  Nothing depends on timing, so two launches give the same bits.  Made for the stride-8 labels the transform is
// computed from (4800 pixels of a 480x640 frame); it reads full-resolution labels too, at one workgroup's bandwidth.
constexpr int NM = 10;

__global__ __launch_bounds__(ST) void label_moments_kernel(const float* __restrict__ labels, long pixels, int ld, int vec,
                                                           double px, double py, double pz, double* __restrict__ partial) {
  __shared__ double tree[NM][ST];
  const int b = blockIdx.x, t = threadIdx.x;
  const float* src = labels + (long)b * pixels * ld;
  double a[NM];
  for (int k = 0; k < NM; ++k) a[k] = 0.0;
  for (long i = t; i < pixels; i += ST) {
    float4 q;
    if (vec) {
      q = *reinterpret_cast<const float4*>(src + i * ld);
    } else {
      q.x = src[i * ld]; q.y = src[i * ld + 1]; q.z = src[i * ld + 2]; q.w = src[i * ld + 3];
    }
    if (q.w == 1.0f) {
      const double dx = (double)q.x - px, dy = (double)q.y - py, dz = (double)q.z - pz;
      a[0] += 1.0;
      a[1] += dx; a[2] += dy; a[3] += dz;
      a[4] += dx * dx; a[5] += dx * dy; a[6] += dx * dz;
      a[7] += dy * dy; a[8] += dy * dz; a[9] += dz * dz;
    }
  }
  for (int k = 0; k < NM; ++k) tree[k][t] = a[k];
  __syncthreads();
  for (int o = ST / 2; o > 0; o >>= 1) {
    if (t < o)
      for (int k = 0; k < NM; ++k) tree[k][t] += tree[k][t + o];
    __syncthreads();
  }
  if (t < NM) partial[b * NM + t] = tree[t][0];
}

bool sized(int B, int H, int W) { return B > 0 && H >= 8 && W >= 8 && H % 8 == 0 && W % 8 == 0 && (long)B * H * W <= (1L << 30); }

}  // namespace

extern "C" int kfn_depth_labels(const kfn_depth_labels_desc* d, const uint16_t* depth, const float* poses, float* labels_out,
                                void* stream) {
  KFN_REQUIRE(d, "kfn_depth_labels: null descriptor");
  KFN_REQUIRE(d->struct_size == (int32_t)sizeof(kfn_depth_labels_desc), "kfn_depth_labels: struct_size %d, expected %d",
              (int)d->struct_size, (int)sizeof(kfn_depth_labels_desc));
  KFN_REQUIRE(sized(d->B, d->H, d->W), "kfn_depth_labels: %dx%dx%d: height and width must be multiples of 8, at least 8",
              d->B, d->H, d->W);
  KFN_REQUIRE(d->stride == 1 || d->stride == 8, "kfn_depth_labels: stride %d is neither 1 nor 8", d->stride);
  KFN_REQUIRE(d->ld_out >= 4 && d->ld_out <= 1024, "kfn_depth_labels: ld_out %d: a pixel of the output holds at least 4 floats", d->ld_out);
  KFN_REQUIRE(depth && poses && labels_out, "kfn_depth_labels: null buffer");
  KFN_REQUIRE(d->raw_min >= 0 && d->raw_max <= 65535 && d->raw_min <= d->raw_max, "kfn_depth_labels: bad validity window [%d, %d]",
              d->raw_min, d->raw_max);
  const int vec = (d->ld_out & 3) == 0;
  KFN_REQUIRE(((uintptr_t)depth & 15) == 0 && ((uintptr_t)poses & 3) == 0 && ((uintptr_t)labels_out & (vec ? 15 : 3)) == 0,
              "kfn_depth_labels: depth must be 16-byte aligned, labels_out 16-byte (ld_out a multiple of 4) or 4-byte aligned");
  LabelArgs a;
  a.depth = depth; a.poses = poses; a.out = labels_out;
  a.B = d->B; a.H = d->H; a.W = d->W; a.s = d->stride; a.ld = d->ld_out; a.vec = vec; a.reg = d->registration != 0;
  a.raw_min = d->raw_min; a.raw_max = d->raw_max;
  a.u = d->u; a.v = d->v; a.inv_fx = d->inv_fx; a.inv_fy = d->inv_fy;
  a.kx = d->kx; a.ky = d->ky; a.ud = d->ud; a.vd = d->vd; a.scale = d->scale;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (d->stride == 1) {
    const long threads = (long)d->B * d->H * (d->W / PX);
    hipLaunchKernelGGL(depth_labels_full_kernel, dim3((unsigned)((threads + ST - 1) / ST)), dim3(ST), 0, st, a);
    KFN_LAUNCH_CHECK("depth_labels_full_kernel");
  } else {
    const long threads = (long)d->B * (d->H / 8) * (d->W / 8);
    hipLaunchKernelGGL(depth_labels_grid_kernel, dim3((unsigned)((threads + ST - 1) / ST)), dim3(ST), 0, st, a);
    KFN_LAUNCH_CHECK("depth_labels_grid_kernel");
  }
  return KFN_OK;
}

extern "C" int kfn_label_moments(const kfn_label_moments_desc* d, const float* labels, double* partial, void* stream) {
  KFN_REQUIRE(d, "kfn_label_moments: null descriptor");
  KFN_REQUIRE(d->struct_size == (int32_t)sizeof(kfn_label_moments_desc), "kfn_label_moments: struct_size %d, expected %d",
              (int)d->struct_size, (int)sizeof(kfn_label_moments_desc));
  KFN_REQUIRE(d->B > 0 && d->h > 0 && d->w > 0 && (long)d->B * d->h * d->w <= (1L << 30), "kfn_label_moments: bad shape %dx%dx%d",
              d->B, d->h, d->w);
  KFN_REQUIRE(d->ld >= 4 && d->ld <= 1024, "kfn_label_moments: ld %d: a label pixel holds at least 4 floats", d->ld);
  KFN_REQUIRE(labels && partial, "kfn_label_moments: null buffer");
  const int vec = (d->ld & 3) == 0;
  KFN_REQUIRE(((uintptr_t)labels & (vec ? 15 : 3)) == 0 && ((uintptr_t)partial & 7) == 0,
              "kfn_label_moments: labels must be 16-byte (ld a multiple of 4) or 4-byte aligned, partial 8-byte aligned");
  hipLaunchKernelGGL(label_moments_kernel, dim3((unsigned)d->B), dim3(ST), 0, reinterpret_cast<hipStream_t>(stream), labels,
                     (long)d->h * d->w, d->ld, vec, d->pivot[0], d->pivot[1], d->pivot[2], partial);
  KFN_LAUNCH_CHECK("label_moments_kernel");
  return KFN_OK;
}
