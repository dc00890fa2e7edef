// kfn_render.hip -- training labels, depth maps and frames rendered from a triangle mesh (gfx950).
// Compiled with -ffp-contract=off: every operation below is one rounded fp32 operation of DESIGN.md 6j, in that order, so a
// numpy float32 restatement (tests/render_ref.py) gives the same bits.  The quotients are IEEE divisions (hipcc's default
// for fp32), there is no transcendental and no floating-point atomic.
//
//   frame b      P = poses[b][0..11], the rows of [R|t], camera to world.  A non-finite entry: nothing is rasterised.
//   vertex p     d = p - t: dx = p.x - P[3], dy = p.y - P[7], dz = p.z - P[11];  camera frame R^T d:
//                X = (P[0] dx + P[4] dy) + P[8] dz;  Y = (P[1] dx + P[5] dy) + P[9] dz;  Z = (P[2] dx + P[6] dy) + P[10] dz
//   triangle t   indices outside [0, V): skipped (stats word 4).  c0, c1, c2 its camera-frame vertices; a non-finite
//                coordinate, or all three Z < near: culled.  Otherwise it passes (word 1); some Z < near: clipped (word 2).
//     plane      e1 = c1 - c0, e2 = c2 - c0; n = e1 x e2, each component (a b) - (c d): nx = e1.y e2.z - e1.z e2.y,
//                ny = e1.z e2.x - e1.x e2.z, nz = e1.x e2.y - e1.y e2.x;  d = (nx c0.x + ny c0.y) + nz c0.z;
//                d == 0 or non-finite: no coverage.  pa = nx / d, pb = ny / d, pc = nz / d: 1/z = pa x' + pb y' + pc on the
//                image plane z = 1, from the UNCLIPPED triangle.
//     polygon    walk k = 0, 1, 2 with cur = c[k], nxt = c[(k+1)%3], inside = (Z >= near): emit cur when inside; when the
//                two differ emit the crossing of I (the inside one) and O: tt = (I.z - near) / (I.z - O.z),
//                (I.x + tt (O.x - I.x), I.y + tt (O.y - I.y), near) -- a function of (I, O), so two triangles sharing the
//                edge get the same bits.  A vertex is projected as it is emitted: sx = (x / z) fx + u, sy = (y / z) fy + v;
//                non-finite: no coverage.  One equal (sx, sy) to the one emitted before it is dropped, and the last one
//                when it equals the first; fewer than 3 left: no coverage.  The polygon has n = 3 or 4 vertices q[k]; it is
//                tested against its n edges, which is the union of its one or two triangles with no diagonal to own.
//     edge k     from q[k] to q[j], j = (k+1)%n, reference m = (j+1)%n.  Canonical direction: A = q[k], B = q[j], swapped
//                when q[k].x > q[j].x or (equal and q[k].y > q[j].y), so that the neighbour across the edge computes the
//                same numbers.  ex = B.x - A.x, ey = B.y - A.y;  g = ex (q[m].y - A.y) - ey (q[m].x - A.x);  s = +1 / -1 by the
//                sign of g; g == 0: no coverage.  tie = (-s ey > 0) or (-s ey == 0 and s ex > 0): the edge is a left edge,
//                or a top edge (y grows downwards) -- the top-left rule.
//     box        the polygon's min / max sx clamped to [0, W - 1], sy to [0, H - 1]; columns ceil(min / stride) ..
//                floor(max / stride), rows likewise (stride is 1 or 8: the quotient is exact).
//   sample       output pixel (r, c) is image pixel px = float(stride c), py = float(stride r).  Per edge
//                e = ex (py - A.y) - ey (px - A.x), tt = s e; covered iff for every edge tt > 0 or (tt == 0 and tie).
//                rx = (px - u) inv_fx, ry = (py - v) inv_fy (the ray of kfn_depth_labels);  w = (pa rx + pb ry) + pc;
//                w > 0 and z = 1 / w <= FLT_MAX: key = bits(z) << 32 | t, 64-bit integer atomic min into zbuf.
//   resolve      key all ones: label (0, 0, 0, 0), depth 0, frame (0, 0, 0).  Else z, t from the key; X = rx z, Y = ry z;
//                q = rint(z / scale) (ties to even); raw_min <= q <= raw_max: depth q and label
//                (((P[4i] X + P[4i+1] Y) + P[4i+2] z) + P[4i+3], i = 0..2; 1); else depth 0 and label (0, 0, 0, 0).
//     colour     c0..c2 as above, f1 = c1 - c0, f2 = c2 - c0, hp = (X, Y, z) - c0; dots (x x + y y) + z z:
//                d11 = f1.f1, d12 = f1.f2, d22 = f2.f2, h1 = hp.f1, h2 = hp.f2;  den = d11 d22 - d12 d12;
//                b1 = (d22 h1 - d12 h2) / den, b2 = (d11 h2 - d12 h1) / den, b0 = (1 - b1) - b2;
//                channel = min(max(rint((b0 k0 + b1 k1) + b2 k2), 0), 255), k the vertices' colours (255 without colours);
//                a NaN becomes 0.  The colour is written whether or not the depth is in the window.
// Launches: clear (every key all ones, stats zero), rasterise, resolve -- no allocation, no synchronisation.
#include "kfn_common.h"
#include <cfloat>

namespace {

constexpr int RT = 256;        // threads of a workgroup, all three kernels
constexpr int REC = 28;        // dwords of a set-up record: 4 edges x (A.x, A.y, ex, ey, s), plane, box, flags
constexpr unsigned long long EMPTY = ~0ull;

struct RenderArgs {
  const float* vertices;
  const uint8_t* colors;
  const int32_t* triangles;
  const float* poses;
  unsigned long long* zbuf;
  float* labels;
  uint16_t* depth;
  uint8_t* frames;
  int32_t* stats;
  int B, V, N, h, w, s, ld, vec;
  int raw_min, raw_max;
  float u, v, inv_fx, inv_fy, fx, fy, near, scale, inv_s;
};

struct V3 {
  float x, y, z;
};

__device__ __forceinline__ bool finite(float x) { return fabsf(x) <= FLT_MAX; }

__device__ __forceinline__ bool load_pose(const RenderArgs& p, int b, float* P) {
  bool ok = true;
  for (int k = 0; k < 12; ++k) {
    P[k] = p.poses[b * 12 + k];
    ok = ok && finite(P[k]);
  }
  return ok;
}

__device__ __forceinline__ V3 to_camera(const float* P, const float* q) {
  const float dx = q[0] - P[3], dy = q[1] - P[7], dz = q[2] - P[11];
  V3 c;
  c.x = (P[0] * dx + P[4] * dy) + P[8] * dz;
  c.y = (P[1] * dx + P[5] * dy) + P[9] * dz;
  c.z = (P[2] * dx + P[6] * dy) + P[10] * dz;
  return c;
}

__device__ __forceinline__ float dot3(V3 a, V3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
__device__ __forceinline__ V3 sub3(V3 a, V3 b) { V3 c; c.x = a.x - b.x; c.y = a.y - b.y; c.z = a.z - b.z; return c; }

// the polygon under construction: projected vertices, without repeats
struct Polygon {
  float x[4], y[4];
  int n;
  bool ok;
};

__device__ __forceinline__ void emit(const RenderArgs& p, Polygon& g, float x, float y, float z) {
  const float sx = (x / z) * p.fx + p.u;
  const float sy = (y / z) * p.fy + p.v;
  if (!(finite(sx) && finite(sy))) g.ok = false;
  if (g.n > 0 && sx == g.x[g.n - 1] && sy == g.y[g.n - 1]) return;
  if (g.n < 4) {
    g.x[g.n] = sx;
    g.y[g.n] = sy;
    ++g.n;
  }
}

__global__ __launch_bounds__(RT) void render_clear_kernel(RenderArgs p) {
  const long total = (long)p.B * p.h * p.w;
  const long id = (long)blockIdx.x * RT + threadIdx.x;
  if (id < total) p.zbuf[id] = EMPTY;
  if (p.stats && id < (long)p.B * 5) p.stats[id] = 0;
}

// Set-up: thread = (frame blockIdx.y, triangle blockIdx.x RT + threadIdx.x).  Walk: each wave takes its 64 records in
// turn and spreads the box's samples over its lanes.
__global__ __launch_bounds__(RT) void render_raster_kernel(RenderArgs p) {
  __shared__ float rec[REC][RT];
  const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63;
  const long tl = (long)blockIdx.x * RT + tid;
  float P[12];
  if (!load_pose(p, b, P)) return;              // the whole workgroup: b is uniform
  int skipped = 0, passed = 0, clipped = 0;
  bool work = false;
  if (tl < p.N) {
    const int* ix = p.triangles + tl * 3;
    const int i0 = ix[0], i1 = ix[1], i2 = ix[2];
    if ((unsigned)i0 >= (unsigned)p.V || (unsigned)i1 >= (unsigned)p.V || (unsigned)i2 >= (unsigned)p.V) {
      skipped = 1;
    } else {
      V3 c[3];
      c[0] = to_camera(P, p.vertices + (long)i0 * 3);
      c[1] = to_camera(P, p.vertices + (long)i1 * 3);
      c[2] = to_camera(P, p.vertices + (long)i2 * 3);
      bool fin = true, in[3];
      for (int k = 0; k < 3; ++k) {
        fin = fin && finite(c[k].x) && finite(c[k].y) && finite(c[k].z);
        in[k] = c[k].z >= p.near;
      }
      if (fin && (in[0] || in[1] || in[2])) {
        passed = 1;
        clipped = !(in[0] && in[1] && in[2]);
        const V3 e1 = sub3(c[1], c[0]), e2 = sub3(c[2], c[0]);
        const float nx = e1.y * e2.z - e1.z * e2.y;
        const float ny = e1.z * e2.x - e1.x * e2.z;
        const float nz = e1.x * e2.y - e1.y * e2.x;
        const float d = (nx * c[0].x + ny * c[0].y) + nz * c[0].z;
        const float pa = nx / d, pb = ny / d, pc = nz / d;
        Polygon g;
        g.n = 0;
        g.ok = d != 0.0f && finite(pa) && finite(pb) && finite(pc);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          const V3 cur = c[k], nxt = c[k == 2 ? 0 : k + 1];
          const bool ic = in[k], inx = in[k == 2 ? 0 : k + 1];
          if (ic) emit(p, g, cur.x, cur.y, cur.z);
          if (ic != inx) {
            const V3 I = ic ? cur : nxt, O = ic ? nxt : cur;
            const float tt = (I.z - p.near) / (I.z - O.z);
            emit(p, g, I.x + tt * (O.x - I.x), I.y + tt * (O.y - I.y), p.near);
          }
        }
        if (g.n > 1 && g.x[g.n - 1] == g.x[0] && g.y[g.n - 1] == g.y[0]) --g.n;
        if (g.n < 3) g.ok = false;
        int ties = 0;
        float mnx = 0.0f, mxx = 0.0f, mny = 0.0f, mxy = 0.0f;
        if (g.ok) {
          mnx = mxx = g.x[0];
          mny = mxy = g.y[0];
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            if (k < g.n) {
              const int j = k + 1 == g.n ? 0 : k + 1, m = j + 1 == g.n ? 0 : j + 1;
              const bool swap = g.x[k] > g.x[j] || (g.x[k] == g.x[j] && g.y[k] > g.y[j]);
              const float ax = swap ? g.x[j] : g.x[k], ay = swap ? g.y[j] : g.y[k];
              const float bx = swap ? g.x[k] : g.x[j], by = swap ? g.y[k] : g.y[j];
              const float ex = bx - ax, ey = by - ay;
              const float gm = ex * (g.y[m] - ay) - ey * (g.x[m] - ax);
              const float s = gm > 0.0f ? 1.0f : -1.0f;
              if (!(gm > 0.0f || gm < 0.0f)) g.ok = false;
              const float ga = -s * ey, gb = s * ex;
              if (ga > 0.0f || (ga == 0.0f && gb > 0.0f)) ties |= 1 << k;
              rec[k * 5 + 0][tid] = ax;
              rec[k * 5 + 1][tid] = ay;
              rec[k * 5 + 2][tid] = ex;
              rec[k * 5 + 3][tid] = ey;
              rec[k * 5 + 4][tid] = s;
              mnx = fminf(mnx, g.x[k]);
              mxx = fmaxf(mxx, g.x[k]);
              mny = fminf(mny, g.y[k]);
              mxy = fmaxf(mxy, g.y[k]);
            }
          }
        }
        if (g.ok) {
          mnx = fmaxf(mnx, 0.0f);
          mny = fmaxf(mny, 0.0f);
          mxx = fminf(mxx, (float)(p.w * p.s - 1));
          mxy = fminf(mxy, (float)(p.h * p.s - 1));
          if (mnx <= mxx && mny <= mxy) {
            const int c_lo = (int)ceilf(mnx * p.inv_s), c_hi = (int)floorf(mxx * p.inv_s);
            const int r_lo = (int)ceilf(mny * p.inv_s), r_hi = (int)floorf(mxy * p.inv_s);
            if (c_lo <= c_hi && r_lo <= r_hi && c_lo >= 0 && r_lo >= 0 && c_hi < p.w && r_hi < p.h) {
              work = true;
              rec[20][tid] = pa;
              rec[21][tid] = pb;
              rec[22][tid] = pc;
              rec[23][tid] = __int_as_float(c_lo);
              rec[24][tid] = __int_as_float(r_lo);
              rec[25][tid] = __int_as_float(c_hi - c_lo + 1);
              rec[26][tid] = __int_as_float(r_hi - r_lo + 1);
              rec[27][tid] = __int_as_float(g.n | (ties << 4));
            }
          }
        }
      }
    }
  }
  if (p.stats) {
    const unsigned long long ms = __ballot(skipped), mp = __ballot(passed), mc = __ballot(clipped);
    if (lane == 0) {
      if (mp) atomicAdd(p.stats + b * 5 + 1, __popcll(mp));
      if (mc) atomicAdd(p.stats + b * 5 + 2, __popcll(mc));
      if (ms) atomicAdd(p.stats + b * 5 + 4, __popcll(ms));
    }
  }
  __syncthreads();
  unsigned long long todo = __ballot(work);
  const int first = tid & ~63;
  unsigned long long* zb = p.zbuf + (long)b * p.h * p.w;
  while (todo) {
    const int src = first + (__ffsll((long long)todo) - 1);
    todo &= todo - 1;
    const float pa = rec[20][src], pb = rec[21][src], pc = rec[22][src];
    const int c_lo = __float_as_int(rec[23][src]), r_lo = __float_as_int(rec[24][src]);
    const int bw = __float_as_int(rec[25][src]), bh = __float_as_int(rec[26][src]);
    const int flags = __float_as_int(rec[27][src]);
    const int n = flags & 15;
    const unsigned tri = (unsigned)(blockIdx.x * RT + src);
    const int total = bw * bh;
    for (int i = lane; i < total; i += 64) {
      const int rr = i / bw;
      const int r = r_lo + rr, c = c_lo + (i - rr * bw);
      const float px = (float)(c * p.s), py = (float)(r * p.s);
      bool covered = true;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (k < n) {
          const float e = rec[k * 5 + 2][src] * (py - rec[k * 5 + 1][src]) - rec[k * 5 + 3][src] * (px - rec[k * 5 + 0][src]);
          const float tt = rec[k * 5 + 4][src] * e;
          covered = covered && (tt > 0.0f || (tt == 0.0f && ((flags >> (4 + k)) & 1)));
        }
      }
      if (covered) {
        const float rx = (px - p.u) * p.inv_fx, ry = (py - p.v) * p.inv_fy;
        const float w = (pa * rx + pb * ry) + pc;
        if (w > 0.0f) {
          const float z = 1.0f / w;
          if (z <= FLT_MAX)
            atomicMin(zb + (long)r * p.w + c, ((unsigned long long)(unsigned)__float_as_int(z) << 32) | tri);
        }
      }
    }
  }
}

__device__ __forceinline__ float channel(float v) { return fminf(fmaxf(rintf(v), 0.0f), 255.0f); }

__global__ __launch_bounds__(RT) void render_resolve_kernel(RenderArgs p) {
  const int b = blockIdx.y, lane = threadIdx.x & 63;
  const int hw = p.h * p.w;
  const long in = (long)blockIdx.x * RT + threadIdx.x;
  float P[12];
  const bool pose_ok = load_pose(p, b, P);
  int covered = 0;
  if (in < hw) {
    const long id = (long)b * hw + in;
    const unsigned long long key = p.zbuf[id];
    float4 lab = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    int raw = 0;
    float col[3] = {0.0f, 0.0f, 0.0f};
    const unsigned tri = (unsigned)key;
    if (pose_ok && key != EMPTY && tri < (unsigned)p.N) {
      covered = 1;
      const int r = (int)(in / p.w), c = (int)(in - (long)r * p.w);
      const float z = __int_as_float((int)(key >> 32));
      const float px = (float)(c * p.s), py = (float)(r * p.s);
      const float X = ((px - p.u) * p.inv_fx) * z;
      const float Y = ((py - p.v) * p.inv_fy) * z;
      const float q = rintf(z / p.scale);
      if (q >= (float)p.raw_min && q <= (float)p.raw_max) {
        raw = (int)q;
        lab.x = ((P[0] * X + P[1] * Y) + P[2] * z) + P[3];
        lab.y = ((P[4] * X + P[5] * Y) + P[6] * z) + P[7];
        lab.z = ((P[8] * X + P[9] * Y) + P[10] * z) + P[11];
        lab.w = 1.0f;
      }
      if (p.frames) {
        const int* ix = p.triangles + (long)tri * 3;
        const int i0 = ix[0], i1 = ix[1], i2 = ix[2];
        if ((unsigned)i0 < (unsigned)p.V && (unsigned)i1 < (unsigned)p.V && (unsigned)i2 < (unsigned)p.V) {
          const V3 c0 = to_camera(P, p.vertices + (long)i0 * 3);
          const V3 c1 = to_camera(P, p.vertices + (long)i1 * 3);
          const V3 c2 = to_camera(P, p.vertices + (long)i2 * 3);
          V3 hit;
          hit.x = X; hit.y = Y; hit.z = z;
          const V3 f1 = sub3(c1, c0), f2 = sub3(c2, c0), hp = sub3(hit, c0);
          const float d11 = dot3(f1, f1), d12 = dot3(f1, f2), d22 = dot3(f2, f2);
          const float h1 = dot3(hp, f1), h2 = dot3(hp, f2);
          const float den = d11 * d22 - d12 * d12;
          const float b1 = (d22 * h1 - d12 * h2) / den;
          const float b2 = (d11 * h2 - d12 * h1) / den;
          const float b0 = (1.0f - b1) - b2;
          for (int k = 0; k < 3; ++k) {
            const float k0 = p.colors ? (float)p.colors[(long)i0 * 3 + k] : 255.0f;
            const float k1 = p.colors ? (float)p.colors[(long)i1 * 3 + k] : 255.0f;
            const float k2 = p.colors ? (float)p.colors[(long)i2 * 3 + k] : 255.0f;
            col[k] = channel((b0 * k0 + b1 * k1) + b2 * k2);
          }
        }
      }
    }
    if (p.labels) {
      float* dst = p.labels + id * p.ld;
      if (p.vec) {
        *reinterpret_cast<float4*>(dst) = lab;
      } else {
        dst[0] = lab.x; dst[1] = lab.y; dst[2] = lab.z; dst[3] = lab.w;
      }
    }
    if (p.depth) p.depth[id] = (uint16_t)raw;
    if (p.frames) {
      uint8_t* dst = p.frames + id * 3;
      dst[0] = (uint8_t)col[0]; dst[1] = (uint8_t)col[1]; dst[2] = (uint8_t)col[2];
    }
  }
  if (p.stats) {
    const unsigned long long mc = __ballot(covered);
    if (lane == 0 && mc) atomicAdd(p.stats + b * 5, __popcll(mc));
    if (in == 0) p.stats[b * 5 + 3] = pose_ok ? 0 : 1;
  }
}

int checked(const kfn_render_desc* d, const char* who) {
  KFN_REQUIRE(d, "%s: null descriptor", who);
  KFN_REQUIRE(d->struct_size == (int32_t)sizeof(kfn_render_desc), "%s: struct_size %d, expected %d", who, (int)d->struct_size,
              (int)sizeof(kfn_render_desc));
  KFN_REQUIRE(d->stride == 1 || d->stride == 8, "%s: stride %d is neither 1 nor 8", who, d->stride);
  KFN_REQUIRE(d->B > 0 && d->V > 0 && d->N > 0 && d->H > 0 && d->W > 0, "%s: sizes must be positive (B %d, V %d, N %d, %dx%d)",
              who, d->B, d->V, d->N, d->H, d->W);
  KFN_REQUIRE(d->B <= 65535, "%s: %d frames: at most 65535 in one call", who, d->B);
  KFN_REQUIRE(d->H % d->stride == 0 && d->W % d->stride == 0, "%s: %dx%d: height and width must be multiples of the stride %d",
              who, d->H, d->W, d->stride);
  KFN_REQUIRE((long)d->B * (d->H / d->stride) * (d->W / d->stride) < (1L << 31), "%s: %d frames of %dx%d samples: 2^31 or more",
              who, d->B, d->H / d->stride, d->W / d->stride);
  KFN_REQUIRE(d->ld_labels >= 4 && d->ld_labels <= 1024, "%s: ld_labels %d: a label holds at least 4 floats", who, d->ld_labels);
  KFN_REQUIRE(d->near > 0.0f && d->near <= FLT_MAX, "%s: near must be positive and finite", who);
  KFN_REQUIRE(d->scale > 0.0f && d->scale <= FLT_MAX, "%s: scale must be positive and finite", who);
  KFN_REQUIRE(d->raw_min >= 0 && d->raw_max <= 65535 && d->raw_min <= d->raw_max, "%s: bad validity window [%d, %d]", who,
              d->raw_min, d->raw_max);
  return KFN_OK;
}

}  // namespace

extern "C" int kfn_render_scratch_bytes(const kfn_render_desc* d, size_t* bytes) {
  const int rc = checked(d, "kfn_render_scratch_bytes");
  if (rc != KFN_OK) return rc;
  KFN_REQUIRE(bytes, "kfn_render_scratch_bytes: null result");
  *bytes = (size_t)d->B * (size_t)(d->H / d->stride) * (size_t)(d->W / d->stride) * sizeof(unsigned long long);
  return KFN_OK;
}

extern "C" int kfn_render(const kfn_render_desc* d, const float* vertices, const uint8_t* colors, const int32_t* triangles,
                          const float* poses, void* zbuf, float* labels, uint16_t* depth, uint8_t* frames, int32_t* stats,
                          void* stream) {
  const int rc = checked(d, "kfn_render");
  if (rc != KFN_OK) return rc;
  KFN_REQUIRE(vertices && triangles && poses && zbuf, "kfn_render: null buffer (vertices, triangles, poses and zbuf are required)");
  const int vec = (d->ld_labels & 3) == 0;
  KFN_REQUIRE(((uintptr_t)vertices & 3) == 0 && ((uintptr_t)triangles & 3) == 0 && ((uintptr_t)poses & 3) == 0 &&
                  ((uintptr_t)zbuf & 7) == 0 && ((uintptr_t)labels & (vec ? 15 : 3)) == 0 && ((uintptr_t)depth & 1) == 0 &&
                  ((uintptr_t)stats & 3) == 0,
              "kfn_render: zbuf must be 8-byte aligned, labels 16-byte (ld_labels a multiple of 4) or 4-byte aligned");
  RenderArgs a;
  a.vertices = vertices; a.colors = colors; a.triangles = triangles; a.poses = poses;
  a.zbuf = static_cast<unsigned long long*>(zbuf); a.labels = labels; a.depth = depth; a.frames = frames; a.stats = stats;
  a.B = d->B; a.V = d->V; a.N = d->N; a.h = d->H / d->stride; a.w = d->W / d->stride; a.s = d->stride;
  a.ld = d->ld_labels; a.vec = vec; a.raw_min = d->raw_min; a.raw_max = d->raw_max;
  a.u = d->u; a.v = d->v; a.inv_fx = d->inv_fx; a.inv_fy = d->inv_fy; a.fx = d->fx; a.fy = d->fy;
  a.near = d->near; a.scale = d->scale; a.inv_s = d->stride == 1 ? 1.0f : 0.125f;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const long samples = (long)a.B * a.h * a.w;
  const long cleared = samples > (long)a.B * 5 ? samples : (long)a.B * 5;
  hipLaunchKernelGGL(render_clear_kernel, dim3((unsigned)((cleared + RT - 1) / RT)), dim3(RT), 0, st, a);
  KFN_LAUNCH_CHECK("render_clear_kernel");
  hipLaunchKernelGGL(render_raster_kernel, dim3((unsigned)(((long)a.N + RT - 1) / RT), (unsigned)a.B), dim3(RT), 0, st, a);
  KFN_LAUNCH_CHECK("render_raster_kernel");
  hipLaunchKernelGGL(render_resolve_kernel, dim3((unsigned)(((long)a.h * a.w + RT - 1) / RT), (unsigned)a.B), dim3(RT), 0, st, a);
  KFN_LAUNCH_CHECK("render_resolve_kernel");
  return KFN_OK;
}
