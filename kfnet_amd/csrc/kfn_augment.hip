// kfn_augment.hip -- the reference's training augmentation of a batch, fused into one gather (gfx950).
// Compiled with -ffp-contract=off: every operation below is one rounded fp32 operation of DESIGN.md 6c, in that order, so a
// numpy float32 restatement (tests/augment_ref.py) gives the same bits.
//   kfn_frame_channel_sums  the per-frame, per-channel sums behind tf.image.adjust_contrast's mean (random_contrast,
//                           KFNet/train.py:179): exact integers.
//   kfn_augment_batch       data_augmentation (KFNet/train.py:168-193): random_brightness + random_contrast on the frames,
//                           then image and label through image_augmentation (KFNet/util.py:123-136): translation (the
//                           identity at crop_size == image_size, :66-86), or tf.contrib.image.rotate (NEAREST) followed by
//                           crop_and_resize (:88-105) or by resize_images + resize_image_with_crop_or_pad (:107-121).
//                           The rotated image is never built: each bilinear tap is fetched through the rotation map.
//                           Frames come back as uint8 for kfn_first_conv_u8; labels only at the pixels the loss reads.
#include "kfn_common.h"

namespace {

constexpr int ST = 256;     // threads of a workgroup, both kernels
constexpr int PX = 4;       // adjacent output pixels per thread of the frame part: 12 bytes, three dwords

typedef __attribute__((ext_vector_type(4))) unsigned u32x4;

// ---- sums ------------------------------------------------------------------------------------------------------------
// A frame is H*W*3 bytes with H, W multiples of 8: a whole number of 16-byte words.  Byte m of word w holds channel
// (w + m) % 3.  A thread walks words tid, tid + T, ... with T a multiple of 3, so its words share one phase: it adds the
// bytes by position class m % 3 and turns the three class sums into channel sums once.
__global__ __launch_bounds__(ST) void channel_sums_kernel(const uint8_t* __restrict__ img, long words, uint32_t* __restrict__ sums) {
  __shared__ uint32_t part[ST / 64][3];
  const int b = blockIdx.y;
  const u32x4* src = reinterpret_cast<const u32x4*>(img + (long)b * words * 16);
  const long first = (long)blockIdx.x * ST + threadIdx.x, step = (long)gridDim.x * ST;   // gridDim.x % 3 == 0
  uint32_t a0 = 0, a1 = 0, a2 = 0;
  for (long w = first; w < words; w += step) {
    const u32x4 v = src[w];
    // classes of the bytes of the four dwords (low byte first): 0120 1201 2012 0120
    a0 = __builtin_amdgcn_sad_u8(v.x & 0xFF0000FFu, 0u, a0);
    a1 = __builtin_amdgcn_sad_u8(v.x & 0x0000FF00u, 0u, a1);
    a2 = __builtin_amdgcn_sad_u8(v.x & 0x00FF0000u, 0u, a2);
    a1 = __builtin_amdgcn_sad_u8(v.y & 0xFF0000FFu, 0u, a1);
    a2 = __builtin_amdgcn_sad_u8(v.y & 0x0000FF00u, 0u, a2);
    a0 = __builtin_amdgcn_sad_u8(v.y & 0x00FF0000u, 0u, a0);
    a2 = __builtin_amdgcn_sad_u8(v.z & 0xFF0000FFu, 0u, a2);
    a0 = __builtin_amdgcn_sad_u8(v.z & 0x0000FF00u, 0u, a0);
    a1 = __builtin_amdgcn_sad_u8(v.z & 0x00FF0000u, 0u, a1);
    a0 = __builtin_amdgcn_sad_u8(v.w & 0xFF0000FFu, 0u, a0);
    a1 = __builtin_amdgcn_sad_u8(v.w & 0x0000FF00u, 0u, a1);
    a2 = __builtin_amdgcn_sad_u8(v.w & 0x00FF0000u, 0u, a2);
  }
  const int phase = (int)(first % 3);          // class k of this thread's words is channel (phase + k) % 3
  uint32_t c0 = phase == 0 ? a0 : phase == 1 ? a2 : a1;
  uint32_t c1 = phase == 0 ? a1 : phase == 1 ? a0 : a2;
  uint32_t c2 = phase == 0 ? a2 : phase == 1 ? a1 : a0;
  for (int o = 32; o > 0; o >>= 1) {           // integer adds: any order gives the same sum
    c0 += __shfl_xor(c0, o);
    c1 += __shfl_xor(c1, o);
    c2 += __shfl_xor(c2, o);
  }
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    part[wave][0] = c0; part[wave][1] = c1; part[wave][2] = c2;
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    uint32_t s = 0;
    for (int k = 0; k < ST / 64; ++k) s += part[k][threadIdx.x];
    atomicAdd(sums + b * 4 + threadIdx.x, s);
  }
}

// ---- the gather --------------------------------------------------------------------------------------------------------
struct AugArgs {
  const uint8_t* fin;
  const float4* lin;
  uint8_t* fout;
  float4* lout;
  const uint32_t* sums;
  int B, H, W, s, mode, has_rot, has_col;
  float rot[6];
  float y0, dy, x0, dx;
  int new_h, new_w, off_y, off_x;
  float scale_y, scale_x;
  float delta, factor;
  unsigned frame_blocks;
};

// One axis of the resampling: the two source lines and the weight of the second, or !ok = the output is the fill value.
struct Axis {
  int lo, hi;
  float frac;
  bool ok;
};

__device__ __forceinline__ Axis resolve(int mode, int i, int size, float o0, float d, int new_n, int off, float scale) {
  Axis a;
  float in;
  if (mode == 1) {   // crop_and_resize: in = y1 (H - 1) + i * height_scale, extrapolation value 0 outside [0, H - 1]
    in = o0 + (float)i * d;
    a.ok = in >= 0.0f && in <= (float)(size - 1);
    const float fl = floorf(in);
    a.lo = (int)fl;
    a.hi = (int)ceilf(in);
    a.frac = in - fl;
  } else {           // resize_bilinear (align_corners off) to new_n lines, then centred zero padding
    const int ii = i - off;
    a.ok = ii >= 0 && ii < new_n;
    in = (float)ii * scale;
    const float fl = floorf(in);
    a.lo = min(max((int)fl, 0), size - 1);
    a.hi = min(a.lo + 1, size - 1);
    a.frac = in - fl;
  }
  if (!a.ok) {
    a.lo = a.hi = 0;
    a.frac = 0.0f;
  }
  return a;
}

// Pixel (x, y) of the rotated image is pixel (qx, qy) of the source, or the fill value (false).
__device__ __forceinline__ bool rotated(const AugArgs& p, int x, int y, int* qx, int* qy) {
  if (!p.has_rot) {
    *qx = x; *qy = y;
    return true;
  }
  const float fx = (float)x, fy = (float)y;
  const float sx = (p.rot[0] * fx + p.rot[1] * fy) + p.rot[2];
  const float sy = (p.rot[3] * fx + p.rot[4] * fy) + p.rot[5];
  const float rx = roundf(sx), ry = roundf(sy);            // half away from zero
  if (!(rx >= 0.0f && rx <= (float)(p.W - 1) && ry >= 0.0f && ry <= (float)(p.H - 1))) return false;
  *qx = (int)rx; *qy = (int)ry;
  return true;
}

__device__ __forceinline__ float lerp2(float tl, float tr, float bl, float br, float lx, float ly) {
  const float top = tl + (tr - tl) * lx;
  const float bot = bl + (br - bl) * lx;
  return top + (bot - top) * ly;
}

__device__ __forceinline__ uint32_t to_u8(float v) { return (uint32_t)fminf(fmaxf(rintf(v), 0.0f), 255.0f); }

struct Colour {
  float mean[3];
  float delta, factor;
  bool on;
};

__device__ __forceinline__ float colour(const Colour& c, int ch, uint8_t v) {
  const float x = (float)v;
  if (!c.on) return x;
  return ((x + c.delta) - c.mean[ch]) * c.factor + c.mean[ch];
}

// PX adjacent pixels of one output row per thread
__device__ __forceinline__ void augment_frames(const AugArgs& p) {
  const int groups = p.W / PX;
  const long total = (long)p.B * p.H * groups;
  const long id = (long)blockIdx.x * ST + threadIdx.x;
  if (id >= total) return;
  const int g = (int)(id % groups);
  const long row = id / groups;
  const int i = (int)(row % p.H), b = (int)(row / p.H);
  const uint8_t* src = p.fin + (long)b * p.H * p.W * 3;
  Colour col;
  col.on = p.has_col != 0;
  col.delta = p.delta; col.factor = p.factor;
  col.mean[0] = col.mean[1] = col.mean[2] = 0.0f;
  if (col.on) {
    const double n = (double)((long)p.H * p.W);
    for (int c = 0; c < 3; ++c) col.mean[c] = (float)((double)p.sums[b * 4 + c] / n + (double)p.delta);
  }
  uint32_t out[PX * 3];
  if (p.mode == 0) {
    for (int k = 0; k < PX; ++k) {
      const uint8_t* t = src + ((long)i * p.W + (g * PX + k)) * 3;
      for (int c = 0; c < 3; ++c) out[k * 3 + c] = to_u8(colour(col, c, t[c]));
    }
  } else {
    const Axis ay = resolve(p.mode, i, p.H, p.y0, p.dy, p.new_h, p.off_y, p.scale_y);
    for (int k = 0; k < PX; ++k) {
      const Axis ax = resolve(p.mode, g * PX + k, p.W, p.x0, p.dx, p.new_w, p.off_x, p.scale_x);
      float tap[4][3];
      for (int q = 0; q < 4; ++q) {
        int qx = 0, qy = 0;
        const bool in = ay.ok && ax.ok && rotated(p, (q & 1) ? ax.hi : ax.lo, (q & 2) ? ay.hi : ay.lo, &qx, &qy);
        const uint8_t* t = src + ((long)qy * p.W + qx) * 3;
        for (int c = 0; c < 3; ++c) tap[q][c] = in ? colour(col, c, t[c]) : 0.0f;     // the fill value is not adjusted
      }
      for (int c = 0; c < 3; ++c)
        out[k * 3 + c] = (ay.ok && ax.ok) ? to_u8(lerp2(tap[0][c], tap[1][c], tap[2][c], tap[3][c], ax.frac, ay.frac)) : 0u;
    }
  }
  uint32_t* dst = reinterpret_cast<uint32_t*>(p.fout + ((long)row * p.W + (long)g * PX) * 3);
  for (int k = 0; k < 3; ++k) dst[k] = out[4 * k] | (out[4 * k + 1] << 8) | (out[4 * k + 2] << 16) | (out[4 * k + 3] << 24);
}

// one thread per label pixel the loss reads: output pixel (s r, s c)
__device__ __forceinline__ void augment_labels(const AugArgs& p) {
  const int h = p.H / p.s, w = p.W / p.s;
  const long total = (long)p.B * h * w;
  const long id = (long)(blockIdx.x - p.frame_blocks) * ST + threadIdx.x;
  if (id >= total) return;
  const int c = (int)(id % w);
  const long rest = id / w;
  const int r = (int)(rest % h), b = (int)(rest / h);
  const int i = r * p.s, j = c * p.s;
  const float4* src = p.lin + (long)b * p.H * p.W;
  float4 v;
  if (p.mode == 0) {
    v = src[(long)i * p.W + j];
  } else {
    const Axis ay = resolve(p.mode, i, p.H, p.y0, p.dy, p.new_h, p.off_y, p.scale_y);
    const Axis ax = resolve(p.mode, j, p.W, p.x0, p.dx, p.new_w, p.off_x, p.scale_x);
    float4 tap[4];
    for (int q = 0; q < 4; ++q) {
      int qx = 0, qy = 0;
      const bool in = ay.ok && ax.ok && rotated(p, (q & 1) ? ax.hi : ax.lo, (q & 2) ? ay.hi : ay.lo, &qx, &qy);
      tap[q] = in ? src[(long)qy * p.W + qx] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
    v.x = lerp2(tap[0].x, tap[1].x, tap[2].x, tap[3].x, ax.frac, ay.frac);
    v.y = lerp2(tap[0].y, tap[1].y, tap[2].y, tap[3].y, ax.frac, ay.frac);
    v.z = lerp2(tap[0].z, tap[1].z, tap[2].z, tap[3].z, ax.frac, ay.frac);
    v.w = lerp2(tap[0].w, tap[1].w, tap[2].w, tap[3].w, ax.frac, ay.frac);
  }
  v.w = v.w >= 1.0f ? 1.0f : 0.0f;       // KFNet/train.py:189
  p.lout[id] = v;
}

__global__ __launch_bounds__(ST) void augment_kernel(AugArgs p) {
  if (blockIdx.x < p.frame_blocks) augment_frames(p);
  else augment_labels(p);
}

// one thread per output pixel (s r, s c): augment_labels with the gathered label replaced by the pixel's own normalised
// coordinates, ((float(qx) - u) inv_fx, (float(qy) - v) inv_fy)
__global__ __launch_bounds__(ST) void pixel_map_kernel(AugArgs p, float u, float v, float inv_fx, float inv_fy, float2* __restrict__ out) {
  const int h = p.H / p.s, w = p.W / p.s;
  const long id = (long)blockIdx.x * ST + threadIdx.x;
  if (id >= (long)h * w) return;
  const int c = (int)(id % w), r = (int)(id / w);
  const int i = r * p.s, j = c * p.s;
  float2 o;
  if (p.mode == 0) {
    o.x = ((float)j - u) * inv_fx;
    o.y = ((float)i - v) * inv_fy;
  } else {
    const Axis ay = resolve(p.mode, i, p.H, p.y0, p.dy, p.new_h, p.off_y, p.scale_y);
    const Axis ax = resolve(p.mode, j, p.W, p.x0, p.dx, p.new_w, p.off_x, p.scale_x);
    float2 tap[4];
    for (int q = 0; q < 4; ++q) {
      int qx = 0, qy = 0;
      const bool in = ay.ok && ax.ok && rotated(p, (q & 1) ? ax.hi : ax.lo, (q & 2) ? ay.hi : ay.lo, &qx, &qy);
      tap[q] = in ? make_float2(((float)qx - u) * inv_fx, ((float)qy - v) * inv_fy) : make_float2(0.0f, 0.0f);
    }
    o.x = lerp2(tap[0].x, tap[1].x, tap[2].x, tap[3].x, ax.frac, ay.frac);
    o.y = lerp2(tap[0].y, tap[1].y, tap[2].y, tap[3].y, ax.frac, ay.frac);
  }
  out[id] = o;
}

bool sized(int B, int H, int W) { return B > 0 && H >= 8 && W >= 8 && H % 8 == 0 && W % 8 == 0 && (long)B * H * W <= (1L << 30); }

// the descriptor's part of the launch arguments: sizes, mode and the constants of the resampling
AugArgs geometry(const kfn_augment_desc* d) {
  AugArgs a;
  a.fin = nullptr; a.lin = nullptr; a.fout = nullptr; a.lout = nullptr; a.sums = nullptr;
  a.B = d->B; a.H = d->H; a.W = d->W; a.s = d->label_stride; a.mode = d->mode;
  a.has_rot = d->mode != 0 && d->has_rotation; a.has_col = d->has_colour;
  for (int i = 0; i < 6; ++i) a.rot[i] = d->rot[i];
  a.y0 = d->y0; a.dy = d->dy; a.x0 = d->x0; a.dx = d->dx;
  a.new_h = d->new_h; a.new_w = d->new_w; a.off_y = d->off_y; a.off_x = d->off_x;
  a.scale_y = d->scale_y; a.scale_x = d->scale_x; a.delta = d->delta; a.factor = d->factor;
  a.frame_blocks = 0;
  return a;
}

}  // namespace

extern "C" int kfn_frame_channel_sums(const uint8_t* img, int B, int H, int W, uint32_t* sums, void* stream) {
  KFN_REQUIRE(img && sums, "kfn_frame_channel_sums: null argument");
  KFN_REQUIRE(sized(B, H, W), "kfn_frame_channel_sums: %dx%dx%d: height and width must be multiples of 8, at least 8", B, H, W);
  KFN_REQUIRE(((uintptr_t)img & 15) == 0 && ((uintptr_t)sums & 3) == 0, "kfn_frame_channel_sums: img must be 16-byte aligned");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  KFN_HIP(hipMemsetAsync(sums, 0, (size_t)B * 4 * sizeof(uint32_t), st));
  const long words = (long)H * W * 3 / 16;
  long blocks = (words + ST * 4 - 1) / (ST * 4);          // about four words per thread
  blocks = (blocks + 2) / 3 * 3;                          // the walk's step is a multiple of three words
  hipLaunchKernelGGL(channel_sums_kernel, dim3((unsigned)blocks, (unsigned)B), dim3(ST), 0, st, img, words, sums);
  KFN_LAUNCH_CHECK("channel_sums_kernel");
  return KFN_OK;
}

extern "C" int kfn_augment_batch(const kfn_augment_desc* d, const uint8_t* frames_in, const float* labels_in, uint8_t* frames_out,
                                 float* labels_out, uint32_t* sums, void* stream) {
  KFN_REQUIRE(d, "kfn_augment_batch: null descriptor");
  KFN_REQUIRE(d->struct_size == (int32_t)sizeof(kfn_augment_desc), "kfn_augment_batch: struct_size %d, expected %d",
              (int)d->struct_size, (int)sizeof(kfn_augment_desc));
  KFN_REQUIRE(sized(d->B, d->H, d->W), "kfn_augment_batch: %dx%dx%d: height and width must be multiples of 8, at least 8",
              d->B, d->H, d->W);
  KFN_REQUIRE(d->label_stride == 1 || d->label_stride == 8, "kfn_augment_batch: label_stride %d is neither 1 nor 8", d->label_stride);
  KFN_REQUIRE(d->mode >= 0 && d->mode <= 2, "kfn_augment_batch: unknown mode %d", d->mode);
  KFN_REQUIRE(frames_in && frames_out, "kfn_augment_batch: null frames");
  KFN_REQUIRE(frames_in != frames_out, "kfn_augment_batch: the gather cannot run in place (frames_out == frames_in)");
  KFN_REQUIRE((labels_in == nullptr) == (labels_out == nullptr), "kfn_augment_batch: labels_in and labels_out go together (both or neither)");
  KFN_REQUIRE(labels_in == nullptr || labels_in != labels_out, "kfn_augment_batch: the gather cannot run in place (labels_out == labels_in)");
  KFN_REQUIRE(!d->has_colour || sums, "kfn_augment_batch: the colour adjustment needs the sums buffer");
  KFN_REQUIRE(((uintptr_t)frames_out & 3) == 0 && ((uintptr_t)labels_in & 15) == 0 && ((uintptr_t)labels_out & 15) == 0,
              "kfn_augment_batch: frames_out must be 4-byte and the labels 16-byte aligned");
  if (d->mode == 2)
    KFN_REQUIRE(d->new_h >= 1 && d->new_h <= d->H && d->new_w >= 1 && d->new_w <= d->W && d->off_y >= 0 && d->off_y <= d->H - d->new_h &&
                d->off_x >= 0 && d->off_x <= d->W - d->new_w && d->scale_y > 0.0f && d->scale_x > 0.0f,
                "kfn_augment_batch: bad shrink constants (new %dx%d at offset %d, %d)", d->new_h, d->new_w, d->off_y, d->off_x);
  if (d->has_colour) {
    const int rc = kfn_frame_channel_sums(frames_in, d->B, d->H, d->W, sums, stream);
    if (rc != KFN_OK) return rc;
  }
  AugArgs a = geometry(d);
  a.fin = frames_in; a.lin = reinterpret_cast<const float4*>(labels_in); a.fout = frames_out;
  a.lout = reinterpret_cast<float4*>(labels_out); a.sums = sums;
  const long frame_threads = (long)d->B * d->H * (d->W / PX);
  const long label_threads = labels_in ? (long)d->B * (d->H / d->label_stride) * (d->W / d->label_stride) : 0;
  a.frame_blocks = (unsigned)((frame_threads + ST - 1) / ST);
  const unsigned label_blocks = (unsigned)((label_threads + ST - 1) / ST);
  hipLaunchKernelGGL(augment_kernel, dim3(a.frame_blocks + label_blocks), dim3(ST), 0, reinterpret_cast<hipStream_t>(stream), a);
  KFN_LAUNCH_CHECK("augment_kernel");
  return KFN_OK;
}

extern "C" int kfn_augment_pixel_map(const kfn_augment_desc* d, float u, float v, float inv_fx, float inv_fy, float* out,
                                     void* stream) {
  KFN_REQUIRE(d && out, "kfn_augment_pixel_map: null argument");
  KFN_REQUIRE(d->struct_size == (int32_t)sizeof(kfn_augment_desc), "kfn_augment_pixel_map: struct_size %d, expected %d",
              (int)d->struct_size, (int)sizeof(kfn_augment_desc));
  KFN_REQUIRE(sized(d->B, d->H, d->W), "kfn_augment_pixel_map: %dx%dx%d: height and width must be multiples of 8, at least 8",
              d->B, d->H, d->W);
  KFN_REQUIRE(d->label_stride == 1 || d->label_stride == 8, "kfn_augment_pixel_map: label_stride %d is neither 1 nor 8", d->label_stride);
  KFN_REQUIRE(d->mode >= 0 && d->mode <= 2, "kfn_augment_pixel_map: unknown mode %d", d->mode);
  KFN_REQUIRE(((uintptr_t)out & 7) == 0, "kfn_augment_pixel_map: out must be 8-byte aligned");
  if (d->mode == 2)
    KFN_REQUIRE(d->new_h >= 1 && d->new_h <= d->H && d->new_w >= 1 && d->new_w <= d->W && d->off_y >= 0 && d->off_y <= d->H - d->new_h &&
                d->off_x >= 0 && d->off_x <= d->W - d->new_w && d->scale_y > 0.0f && d->scale_x > 0.0f,
                "kfn_augment_pixel_map: bad shrink constants (new %dx%d at offset %d, %d)", d->new_h, d->new_w, d->off_y, d->off_x);
  const AugArgs a = geometry(d);
  const long cells = (long)(d->H / d->label_stride) * (d->W / d->label_stride);
  hipLaunchKernelGGL(pixel_map_kernel, dim3((unsigned)((cells + ST - 1) / ST)), dim3(ST), 0, reinterpret_cast<hipStream_t>(stream), a,
                     u, v, inv_fx, inv_fy, reinterpret_cast<float2*>(out));
  KFN_LAUNCH_CHECK("pixel_map_kernel");
  return KFN_OK;
}
