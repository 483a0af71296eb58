// Elastic and affine augmentation of a network-size sample (include/cfun_sample_warp.h): a trilinear control-grid displacement,
// an in-plane affine map and per-axis flips, applied to a dense float32 [D,H,W] image (order 0 or 1) and dense uint8 labels
// (order 0), with the GT box of the warped labels.
//   (a) k_warp_gather<ORDER>  one gather over the OUTPUT: control coordinate, displacement from LDS, map, flips, one label tap and
//                             one (ORDER 0) or eight (ORDER 1) image taps per voxel, per-workgroup min / max of z, y, x over
//                             label != 0.  Two instantiations: the order-0 form has no tap arithmetic in it at all.
//   (b) k_warp_finish         one workgroup: partials -> box, 5 % expansion, empty flag (sample.hip's k_box_finish rule)
// No atomics: the box goes through per-workgroup partials, so two runs agree bit for bit.  Built without FMA contraction: the
// rule is an exact contract with tests/sample_warp_ref.py (the same double operations in the same order).
//
// Tile of (a).  Source and output are both x-fastest, so there is no re-layout and no transpose tile: every thread owns a QUAD
// of four consecutive output x and stores it straight from registers -- 16 B of image and 4 B of labels when W % 4 == 0 and the
// pointers are aligned, four guarded scalar stores otherwise.  What is left to choose is the output BRICK of a workgroup, and
// what decides it is how compact its source footprint is: at 20 degrees a 64-wide output row skews over about 22 source rows,
// a 32-wide one over about 11.  The brick is kWX = 32 x (8 quads) by kWY = 8 y by kWZ = 4 z: a wave is one z plane of it, a
// 32 x 8 patch whose rotated footprint is about (32 + 8 sin) x (8 + 32 sin), i.e. 35 x 19 source voxels at 20 degrees (28 rows of
// 128-byte lines at most, each shared by neighbouring output rows of the same wave), against 64 x 4 -> 62 x 26; the four planes
// of a workgroup re-use the same lines of the neighbouring source planes for order 1 (a z tap pair) and under a z displacement.
// Lanes of one row read their quads 16 B apart, so the four loads of a quad fall into the same lines one after the other and
// are served by the CU's cache; neighbouring bricks along x are neighbouring workgroup ids, which share the L2 lines across
// the skew.  The rate this gives is a measurement (profiles/sample_warp_pipeline.txt), not a property of
// the tile.
//
// Control values.  The control cell of a voxel is monotone in its index, so a brick needs the control points from the cell of
// its first voxel to the cell of its last one + 1 per axis: usually 2-3 points per axis (a 5^3 grid over 192 x 320 x 320 has
// cells of 48 x 80 x 80 voxels), staged ONCE per workgroup into LDS as a compact [3][cz][cy][cx] block and read from there by
// every lane (eight ds reads per component; neighbouring lanes read the same words: broadcasts).  A grid finer than the
// volume puts the whole grid under one brick, so LDS holds 3 * kMaxGrid^3 floats: kMaxGrid = 12 -> 20.25 KB, which still lets
// seven workgroups share a CU's 160 KB -- more than the registers of the order-1 form allow anyway.
#include <limits.h>
#include <math.h>

#include "common.h"
#include "../../include/cfun_sample_warp.h"

namespace {

constexpr int kNT = 256;
constexpr int kWX = 32, kWY = 8, kWZ = 4, kMaxGrid = 12;      // warp brick: a quad of x per thread, a z plane per wave; largest control-grid extent
static_assert((kWX / 4) * kWY * kWZ == kNT, "one quad per thread");
static_assert((kWX / 4) * kWY == 64, "a wave is one z plane of the brick");

__device__ __forceinline__ int wave_min_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { const int n = __shfl_xor(v, o, 64); v = n < v ? n : v; }
  return v;
}
__device__ __forceinline__ int wave_max_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { const int n = __shfl_xor(v, o, 64); v = n > v ? n : v; }
  return v;
}

// {zmin, zmax, ymin, ymax, xmin, xmax} of the calling workgroup's threads -> out[0..5] (thread 0 writes); empty = {INT_MAX, -1, ..}
__device__ __forceinline__ void block_minmax6(int (&v)[6], int* __restrict__ out) {
  __shared__ int red[kNT / 64][6];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < 6; ++k) v[k] = (k & 1) ? wave_max_i(v[k]) : wave_min_i(v[k]);
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < 6; ++k) red[wave][k] = v[k];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      int r = red[0][k];
      for (int w = 1; w < kNT / 64; ++w) r = (k & 1) ? (red[w][k] > r ? red[w][k] : r) : (red[w][k] < r ? red[w][k] : r);
      out[k] = r;
    }
  }
}

struct WarpArgs {
  int n[3];                  // D, H, W
  int g[3];                  // gz, gy, gx (2 without a grid)
  double q[3];               // (double)(g - 1) / (double)(n - 1) per axis, 0 when n == 1
  double map[6];
  int ntx, nty;              // bricks along x and y
  int has_grid, has_map, flips;
};

// step 1 on one axis: the control cell i and the weight t of output index o
__device__ __forceinline__ int control_cell(int o, double q, int g, double& t) {
  const double u = (double)o * q;
  const double fl = floor(u);
  const double i = fl < (double)(g - 2) ? fl : (double)(g - 2);
  t = u - i;
  return (int)i;
}

__device__ __forceinline__ double lerp(double a, double b, double t) { return (1.0 - t) * a + t * b; }

// (long long)(v > 0 ? v + 0.5 : v - 0.5), kept in double: the range test comes before any cast
__device__ __forceinline__ double round_half_away(double v) { return trunc(v > 0.0 ? v + 0.5 : v - 0.5); }

template <int ORDER>
__global__ void __launch_bounds__(kNT)
k_warp_gather(const float* __restrict__ img, const uint8_t* __restrict__ lab, const float* __restrict__ grid,
              float* __restrict__ oimg, uint8_t* __restrict__ olab, int32_t* __restrict__ partials, WarpArgs a, int vec) {
  __shared__ float cg[3 * kMaxGrid * kMaxGrid * kMaxGrid];
  const int t = threadIdx.x;
  const int D = a.n[0], H = a.n[1], W = a.n[2];
  const int bid = (int)blockIdx.x;
  const int x0 = (bid % a.ntx) * kWX, y0 = ((bid / a.ntx) % a.nty) * kWY, z0 = (bid / (a.ntx * a.nty)) * kWZ;

  // the control points this brick needs: from the cell of its first voxel to the cell of its last one + 1, per axis
  int lo[3] = {0, 0, 0}, cnt[3] = {2, 2, 2};
  if (a.has_grid) {
    const int first[3] = {z0, y0, x0};
    const int last[3] = {(z0 + kWZ < D ? z0 + kWZ : D) - 1, (y0 + kWY < H ? y0 + kWY : H) - 1, (x0 + kWX < W ? x0 + kWX : W) - 1};
    double unused;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      lo[k] = control_cell(first[k], a.q[k], a.g[k], unused);
      cnt[k] = control_cell(last[k], a.q[k], a.g[k], unused) + 2 - lo[k];      // 2 .. g: at most kMaxGrid
    }
    const int plane = cnt[1] * cnt[2], block = cnt[0] * plane;
    for (int e = t; e < 3 * block; e += kNT) {
      const int c = e / block, r = e - c * block;
      const int kz = r / plane, r2 = r - kz * plane;
      const int ky = r2 / cnt[2], kx = r2 - ky * cnt[2];
      cg[e] = grid[(((long long)c * a.g[0] + lo[0] + kz) * a.g[1] + lo[1] + ky) * a.g[2] + lo[2] + kx];
    }
    __syncthreads();
  }

  const int x4 = x0 + (t & 7) * 4, y = y0 + ((t >> 3) & 7), z = z0 + (t >> 6);
  float out[4] = {0.f, 0.f, 0.f, 0.f};
  uint32_t lpack = 0;
  int mm[6] = {INT_MAX, -1, INT_MAX, -1, INT_MAX, -1};
  const bool live = z < D && y < H && x4 < W;
  if (live) {
    double tz = 0.0, ty = 0.0;
    int cz = 0, cy = 0;
    if (a.has_grid) {
      cz = control_cell(z, a.q[0], a.g[0], tz) - lo[0];
      cy = control_cell(y, a.q[1], a.g[1], ty) - lo[1];
    }
    const int plane = cnt[1] * cnt[2], block = cnt[0] * plane;
    const long long HW = (long long)H * W;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int x = x4 + j;
      if (x >= W) break;                                 // (only without vec: W % 4 != 0)
      double p[3] = {(double)z, (double)y, (double)x};
      if (a.has_grid) {                                  // steps 1 to 3
        double tx;
        const int cx = control_cell(x, a.q[2], a.g[2], tx) - lo[2];
        const float* base = cg + (cz * cnt[1] + cy) * cnt[2] + cx;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const float* v = base + c * block;
          const double e00 = lerp((double)v[0], (double)v[1], tx);
          const double e01 = lerp((double)v[cnt[2]], (double)v[cnt[2] + 1], tx);
          const double e10 = lerp((double)v[plane], (double)v[plane + 1], tx);
          const double e11 = lerp((double)v[plane + cnt[2]], (double)v[plane + cnt[2] + 1], tx);
          const double f0 = lerp(e00, e01, ty), f1 = lerp(e10, e11, ty);
          p[c] = p[c] + lerp(f0, f1, tz);
        }
      }
      double s[3] = {p[0], p[1], p[2]};
      if (a.has_map) {                                   // step 4
        s[2] = a.map[0] * p[2] + a.map[1] * p[1] + a.map[2];
        s[1] = a.map[3] * p[2] + a.map[4] * p[1] + a.map[5];
      }
#pragma unroll
      for (int k = 0; k < 3; ++k)                        // step 5
        if (a.flips & (1 << k)) s[k] = (double)(a.n[k] - 1) - s[k];
      // step 6: the nearest source voxel; a NaN fails every comparison
      const double rz = round_half_away(s[0]), ry = round_half_away(s[1]), rx = round_half_away(s[2]);
      int l = 0;
      if (rz >= 0.0 && rz < (double)D && ry >= 0.0 && ry < (double)H && rx >= 0.0 && rx < (double)W) {
        const long long o = (long long)rz * HW + (long long)ry * W + (long long)rx;
        l = (int)lab[o];
        if (ORDER == 0) out[j] = img[o];
      }
      if (ORDER == 1) {                                  // step 7
        if (s[0] > -1.0 && s[0] < (double)D && s[1] > -1.0 && s[1] < (double)H && s[2] > -1.0 && s[2] < (double)W) {
          const double bz = floor(s[0]), by = floor(s[1]), bx = floor(s[2]);
          const double fz = s[0] - bz, fy = s[1] - by, fx = s[2] - bx;
          const int iz = (int)bz, iy = (int)by, ix = (int)bx;         // -1 .. n - 1
          const bool inz[2] = {iz >= 0, iz + 1 < D}, iny[2] = {iy >= 0, iy + 1 < H}, inx[2] = {ix >= 0, ix + 1 < W};
          // a tap outside the source is loaded from a clamped (valid) address and dropped by a select: eight unconditional loads
          const long long oz[2] = {(long long)(inz[0] ? iz : 0) * HW, (long long)(inz[1] ? iz + 1 : iz) * HW};
          const long long oy[2] = {(long long)(iny[0] ? iy : 0) * W, (long long)(iny[1] ? iy + 1 : iy) * W};
          const long long ox[2] = {(long long)(inx[0] ? ix : 0), (long long)(inx[1] ? ix + 1 : ix)};
          double v[8];
#pragma unroll
          for (int q = 0; q < 8; ++q) {
            const int dz = q >> 2, dy = (q >> 1) & 1, dx = q & 1;
            const float r = img[oz[dz] + oy[dy] + ox[dx]];
            v[q] = (inz[dz] && iny[dy] && inx[dx]) ? (double)r : 0.0;
          }
          const double f0 = lerp(lerp(v[0], v[1], fx), lerp(v[2], v[3], fx), fy);
          const double f1 = lerp(lerp(v[4], v[5], fx), lerp(v[6], v[7], fx), fy);
          out[j] = (float)lerp(f0, f1, fz);
        }
      }
      lpack |= (uint32_t)l << (8 * j);
      if (l != 0) {
        mm[0] = z; mm[1] = z; mm[2] = y; mm[3] = y;
        mm[4] = x < mm[4] ? x : mm[4]; mm[5] = x > mm[5] ? x : mm[5];
      }
    }
    const long long o = ((long long)z * H + y) * W + x4;
    if (vec) {                                           // W % 4 == 0, aligned outputs: the whole quad lies inside
      *reinterpret_cast<float4*>(oimg + o) = make_float4(out[0], out[1], out[2], out[3]);
      *reinterpret_cast<uint32_t*>(olab + o) = lpack;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (x4 + j < W) {
          oimg[o + j] = out[j];
          olab[o + j] = (uint8_t)(lpack >> (8 * j));
        }
      }
    }
  }
  block_minmax6(mm, partials + (long long)bid * 6);
}

__global__ void __launch_bounds__(kNT)
k_warp_finish(const int32_t* __restrict__ partials, int n, int H, int W, int D, int32_t* __restrict__ raw_box,
              int32_t* __restrict__ box, int32_t* __restrict__ empty) {
  __shared__ int total[6];
  int mm[6] = {INT_MAX, -1, INT_MAX, -1, INT_MAX, -1};
  for (int i = threadIdx.x; i < n; i += kNT) {
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      const int p = partials[(long long)i * 6 + k];
      mm[k] = (k & 1) ? (p > mm[k] ? p : mm[k]) : (p < mm[k] ? p : mm[k]);
    }
  }
  block_minmax6(mm, total);
  if (threadIdx.x == 0) {
    int b[6] = {0, 0, 0, 0, 0, 0};
    const int none = total[1] < 0;
    if (!none && total[0] != total[1]) {       // utils.extract_bboxes: a one-plane object (z1 == z2) gives the zero box
      b[0] = total[0]; b[1] = total[2]; b[2] = total[4];
      b[3] = total[1] + 1; b[4] = total[3] + 1; b[5] = total[5] + 1;
    }
    const int dim[3] = {D, H, W};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      raw_box[k] = b[k];
      raw_box[k + 3] = b[k + 3];
      const double e = (double)(b[k + 3] - b[k]) * 0.05;
      const double lo = (double)b[k] - e, hi = (double)b[k + 3] + e;
      box[k] = (int32_t)floor(lo > 0.0 ? lo : 0.0);
      box[k + 3] = (int32_t)ceil(hi < (double)dim[k] ? hi : (double)dim[k]);
    }
    *empty = none;
  }
}

// bricks of a volume of extent {D, H, W}, or -1 for a bad extent or 2^31 or more voxels (then the count fits an int as well)
long long warp_bricks(const int32_t* n) {
  if (!n || n[0] <= 0 || n[1] <= 0 || n[2] <= 0) return -1;
  if ((long long)n[0] * n[1] > (long long)INT_MAX || (long long)n[0] * n[1] * n[2] > (long long)INT_MAX) return -1;
  return (long long)((n[2] - 1) / kWX + 1) * ((n[1] - 1) / kWY + 1) * ((n[0] - 1) / kWZ + 1);
}

bool overlaps(const void* p, size_t pn, const void* q, size_t qn) {
  const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
  return q != nullptr && a < b + qn && b < a + pn;
}

}  // namespace

extern "C" size_t cfun_sample_warp_workspace_bytes(const int32_t* dims) {
  const long long nb = warp_bricks(dims);
  return nb < 0 ? 0 : (size_t)nb * 6 * sizeof(int32_t);
}

extern "C" int32_t cfun_sample_warp_max_grid(void) { return kMaxGrid; }

extern "C" int cfun_sample_warp(const float* image, const uint8_t* labels, const int32_t* dims, const float* grid,
                                const int32_t* gdims, const double* map, int32_t flips, int32_t image_order, float* out_image,
                                uint8_t* out_labels, int32_t* raw_box, int32_t* box, int32_t* empty, void* workspace,
                                size_t workspace_bytes, cfun_stream_t stream) {
  if (!image || !labels || !dims || !out_image || !out_labels || !raw_box || !box || !empty) return CFUN_EINVAL;
  if (grid && !gdims) return CFUN_EINVAL;
  if (image_order != 0 && image_order != 1) return CFUN_EINVAL;
  if (flips < 0 || flips > 7) return CFUN_EINVAL;
  const long long nb = warp_bricks(dims);
  if (nb < 0) return CFUN_EINVAL;
  WarpArgs a;
  size_t gcount = 3;
  for (int k = 0; k < 3; ++k) {
    a.n[k] = dims[k];
    a.g[k] = grid ? gdims[k] : 2;
    if (a.g[k] < 2 || a.g[k] > kMaxGrid) return CFUN_EINVAL;
    a.q[k] = a.n[k] == 1 ? 0.0 : (double)(a.g[k] - 1) / (double)(a.n[k] - 1);
    gcount *= (size_t)a.g[k];
  }
  a.has_map = map != nullptr;
  for (int k = 0; k < 6; ++k) {
    a.map[k] = map ? map[k] : 0.0;
    if (!isfinite(a.map[k])) return CFUN_EINVAL;
  }
  const size_t count = (size_t)a.n[0] * a.n[1] * a.n[2];
  const void* outs[2] = {out_image, out_labels};
  const size_t out_bytes[2] = {count * sizeof(float), count};
  for (int k = 0; k < 2; ++k) {
    if (overlaps(outs[k], out_bytes[k], image, count * sizeof(float)) || overlaps(outs[k], out_bytes[k], labels, count) ||
        overlaps(outs[k], out_bytes[k], grid, gcount * sizeof(float)))
      return CFUN_EINVAL;
  }
  if (!workspace || workspace_bytes < (size_t)nb * 6 * sizeof(int32_t)) return CFUN_EWORKSPACE;
  a.ntx = (a.n[2] - 1) / kWX + 1;
  a.nty = (a.n[1] - 1) / kWY + 1;
  a.has_grid = grid != nullptr;
  a.flips = flips;
  int32_t* partials = (int32_t*)workspace;
  const int vec = (a.n[2] % 4 == 0) && cfun_aligned16(out_image) && (((uintptr_t)out_labels) & 3) == 0;
  hipStream_t st = cfun_st(stream);
  if (image_order == 0)
    hipLaunchKernelGGL(k_warp_gather<0>, dim3((unsigned)nb), dim3(kNT), 0, st, image, labels, grid, out_image, out_labels, partials, a, vec);
  else
    hipLaunchKernelGGL(k_warp_gather<1>, dim3((unsigned)nb), dim3(kNT), 0, st, image, labels, grid, out_image, out_labels, partials, a, vec);
  CFUN_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_warp_finish, dim3(1), dim3(kNT), 0, st, (const int32_t*)partials, (int)nb, a.n[1], a.n[2], a.n[0], raw_box,
                     box, empty);
  CFUN_LAUNCH_CHECK();
  return CFUN_OK;
}
