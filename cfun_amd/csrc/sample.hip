// Training samples on the device (include/cfun_sample.h): the reference's load_image_gt (model.py:1007-1181) without the host.
//   (a) k_rotate_relay   per-slice nearest rotation of image and label, [H,W,D] -> [D,H,W], label cast to uint8, and the
//                        per-workgroup min / max of z, y, x over label > 0 -- one pass over the volume (8 B read, 5 B
//                        written per voxel; the measured rates are in DESIGN.md section 7 and profiles/sample_pipeline.txt)
//   (b) k_box_finish     partials -> utils.extract_bboxes' box, the 5 % expansion (model.py:1059-1075), the empty flag
//   (c) k_rpn_*          build_rpn_targets (model.py:1090-1181): IoU in double, arg-max per anchor and per GT, the match rule,
//                        the two subsamplings as a (key, index) radix select, the deltas of the kept positives
//   (d) k_lits_gather    the LiTS fork's sample (include/cfun_sample_lits.h): normalise, zero frame, per-slice affine map,
//                        nearest resize, re-layout, label cast and the partials of (b) in one gather pass over the output
// Every grid-wide result goes through per-workgroup partials and a finish launch; the only atomics are integer adds on LDS
// histograms, so every output is repeatable bit for bit.  Built without FMA contraction: the rotation's source index and the
// IoU comparisons are exact contracts with tests/sample_ref.py (same double operations in the same order).
//
// What the reference does NOT pin: imgaug (and its cv2 / scikit-image backends) is not available to this project's
// environments, so parity of the rotation with iaa.Affine(rotate, order = 0) is unpinned, exactly as the order-1 resize is
// (resize.hip).  The rule follows imgaug's documented construction -- rotation about size / 2 - 0.5, nearest sample, constant 0
// outside -- but rounding at exact half-voxel ties and cv2's fixed-point coordinates may differ by one voxel along edges.
//
// Tile of (a): the source's fastest axis is z, the output's is x.  A workgroup owns one output row y, 64 x, 64 z.  Each wave
// reads, per source pixel (iy, ix), the 64-long run along z (256 B, coalesced) and stores it as a COLUMN of a [64 z][65] LDS
// tile (pitch 65 dwords: ds_write_b32 banks are (a / 4) % 32, lane = z -> 32 distinct banks per half-wave); rows of the tile
// are then written along x, 16 B per lane when W % 4 == 0 (the four ds_read_b32 of a quad are 2-way conflicted at this pitch:
// 8 LDS cycles per 1 KiB stored by this count, which is expected to stay below the HBM time of the same bytes but has not been
// confirmed with counters), 4 B per lane otherwise.  A wave has only two 256-byte loads in flight before a dependent LDS store,
// so the pass is not HBM-bound by construction: its rate is a measurement, not a property of the tile.
#include <limits.h>
#include <math.h>

#include "common.h"
#include "../../include/cfun_sample.h"
#include "../../include/cfun_sample_lits.h"

namespace {

constexpr int kNT = 256;
constexpr int kTX = 64, kTZ = 64, kPitch = 65;
constexpr long long kOutside = LLONG_MIN;

struct RotArgs {
  int64_t is[3], ls[3];      // element strides of image / label along H, W, D
  int H, W, D;
  double c, s;
  int rotate;
};

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

__global__ void __launch_bounds__(kNT)
k_rotate_relay(const float* __restrict__ img, const int32_t* __restrict__ lab, float* __restrict__ oimg,
               uint8_t* __restrict__ olab, int32_t* __restrict__ partials, RotArgs a, int vec) {
  __shared__ float timg[kTZ * kPitch];
  __shared__ int tlab[kTZ * kPitch];
  __shared__ long long off_i[kTX], off_l[kTX];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int x0 = blockIdx.x * kTX, y = blockIdx.y, z0 = blockIdx.z * kTZ;

  if (t < kTX) {                       // the source pixel of each output x of this row: once per workgroup, in double
    const int x = x0 + t;
    long long oi = kOutside, ol = kOutside;
    if (x < a.W) {
      double fx = (double)x, fy = (double)y;
      if (a.rotate) {
        const double cy = (double)a.H / 2.0 - 0.5, cx = (double)a.W / 2.0 - 0.5;
        const double dx = (double)x - cx, dy = (double)y - cy;
        const double sx = a.c * dx + a.s * dy + cx;
        const double sy = -a.s * dx + a.c * dy + cy;
        fx = floor(sx + 0.5);
        fy = floor(sy + 0.5);
      }
      if (fx >= 0.0 && fx < (double)a.W && fy >= 0.0 && fy < (double)a.H) {
        const long long ix = (long long)fx, iy = (long long)fy;
        oi = iy * a.is[0] + ix * a.is[1];
        ol = iy * a.ls[0] + ix * a.ls[1];
      }
    }
    off_i[t] = oi;
    off_l[t] = ol;
  }
  __syncthreads();

  const int z = z0 + lane;
  int mm[6] = {INT_MAX, -1, INT_MAX, -1, INT_MAX, -1};
  for (int xi = wave; xi < kTX; xi += kNT / 64) {
    const long long oi = off_i[xi], ol = off_l[xi];
    float v = 0.f;
    int l = 0;
    if (z < a.D && oi != kOutside) {
      v = img[oi + (long long)z * a.is[2]];
      l = lab[ol + (long long)z * a.ls[2]];
    }
    timg[lane * kPitch + xi] = v;
    tlab[lane * kPitch + xi] = l;
    if (l > 0) {
      const int x = x0 + xi;
      mm[0] = z < mm[0] ? z : mm[0]; mm[1] = z > mm[1] ? z : mm[1];
      mm[2] = y; mm[3] = y;
      mm[4] = x < mm[4] ? x : mm[4]; mm[5] = x > mm[5] ? x : mm[5];
    }
  }
  __syncthreads();

  if (vec) {                           // W % 4 == 0, 16-byte aligned outputs: a quad of x per lane
    const int x4 = (t & 15) * 4;
    if (x0 + x4 < a.W) {
      for (int zz = t >> 4; zz < kTZ; zz += kNT / 16) {
        const int zo = z0 + zz;
        if (zo >= a.D) break;
        const long long o = ((long long)zo * a.H + y) * a.W + x0 + x4;
        const float* r = timg + zz * kPitch + x4;
        const int* q = tlab + zz * kPitch + x4;
        *reinterpret_cast<float4*>(oimg + o) = make_float4(r[0], r[1], r[2], r[3]);
        *reinterpret_cast<uint32_t*>(olab + o) = (uint32_t)(q[0] & 255) | ((uint32_t)(q[1] & 255) << 8) |
                                                 ((uint32_t)(q[2] & 255) << 16) | ((uint32_t)(q[3] & 255) << 24);
      }
    }
  } else if (x0 + lane < a.W) {
    for (int zz = wave; zz < kTZ; zz += kNT / 64) {
      const int zo = z0 + zz;
      if (zo >= a.D) break;
      const long long o = ((long long)zo * a.H + y) * a.W + x0 + lane;
      oimg[o] = timg[zz * kPitch + lane];
      olab[o] = (uint8_t)tlab[zz * kPitch + lane];
    }
  }

  const int wg = ((int)blockIdx.z * (int)gridDim.y + (int)blockIdx.y) * (int)gridDim.x + (int)blockIdx.x;
  block_minmax6(mm, partials + (long long)wg * 6);
}

__global__ void __launch_bounds__(kNT)
k_box_finish(const int32_t* __restrict__ partials, int n, int H, int W, int D, int32_t* __restrict__ raw_box,
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

// ------------------------------------------------------------------------------- the LiTS sample (cfun_sample_lits.h)
// Dataset.__getitem__ of the fork (LiTS_2017/model.py:1145-1248) as one gather: every output voxel of normalise -> centre in
// the zero frame -> rotate per slice -> nearest-resize depends on exactly one source voxel, so the 646x646x536 frames are
// never built.  k_rotate_relay's tile carries over (one output row y, 64 x, 64 z; columns through the [64][65] LDS tile; rows
// out as 16-byte stores); new is that the source z of each of the 64 output z is a map as well, computed once per workgroup
// next to the 64 source pixels.  Each lane READS ITS OWN STRIDED ELEMENT along z (stride P_D / D', about 2.1 at the product
// shape) rather than the contiguous run followed by a select: the stride stays far below a 32-byte sector, so both forms pull
// the same sectors from HBM, and the direct read needs no run buffer whose length depends on the ratio (an up-sampling
// shares one source z among several lanes; a steep down-sampling would need a run of any length).  What the stride costs
// is sectors fetched per byte used -- a measurement (profiles/sample_lits_pipeline.txt), not hidden by either form.
struct LitsArgs {
  int64_t is[3], ls[3];      // element strides of image / label along H, W, D
  int n[3];                  // source extent H, W, D
  int P[3];                  // frame extent
  int off[3];                // the source's position in the frame
  int m[3];                  // output extent H', W', D'
  double map[6];
  int has_map, normalise, lab_bytes;
};

// cfun_resize3d's order-0 index (resize.hip)
__device__ __forceinline__ int frame_index(int o, int P, int m) {
  const int k = (int)floor(((double)o + 0.5) * ((double)P / (double)m));
  return k < 0 ? 0 : (k > P - 1 ? P - 1 : k);
}

// (long long)(v > 0 ? v + 0.5 : v - 0.5), kept in double: the range test comes before any cast
__device__ __forceinline__ double round_half_away(double v) { return trunc(v > 0.0 ? v + 0.5 : v - 0.5); }

__global__ void __launch_bounds__(kNT)
k_lits_gather(const float* __restrict__ img, const void* __restrict__ lab, float* __restrict__ oimg, uint8_t* __restrict__ olab,
              int32_t* __restrict__ partials, LitsArgs a, int vec) {
  __shared__ float timg[kTZ * kPitch];
  __shared__ int tlab[kTZ * kPitch];
  __shared__ long long off_i[kTX], off_l[kTX];
  __shared__ int src_z[kTZ];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int x0 = blockIdx.x * kTX, y = blockIdx.y, z0 = blockIdx.z * kTZ;
  const int Hs = a.n[0], Ws = a.n[1], Ds = a.n[2], Ho = a.m[0], Wo = a.m[1], Do = a.m[2];

  if (t < kTX) {                       // the source pixel of each output x of this row: once per workgroup, in double
    const int x = x0 + t;
    long long oi = kOutside, ol = kOutside;
    if (x < Wo) {
      const double fx = (double)frame_index(x, a.P[1], Wo), fy = (double)frame_index(y, a.P[0], Ho);
      double col = fx, row = fy;
      if (a.has_map) {
        col = round_half_away(a.map[0] * fx + a.map[1] * fy + a.map[2]);
        row = round_half_away(a.map[3] * fx + a.map[4] * fy + a.map[5]);
      }
      if (col >= 0.0 && col < (double)a.P[1] && row >= 0.0 && row < (double)a.P[0]) {
        const long long ix = (long long)col - a.off[1], iy = (long long)row - a.off[0];
        if (ix >= 0 && ix < Ws && iy >= 0 && iy < Hs) {
          oi = iy * a.is[0] + ix * a.is[1];
          ol = iy * a.ls[0] + ix * a.ls[1];
        }
      }
    }
    off_i[t] = oi;
    off_l[t] = ol;
  } else if (t < kTX + kTZ) {          // the source z of each output z of this tile: once per workgroup as well
    const int zo = z0 + (t - kTX);
    int sz = -1;
    if (zo < Do) {
      const int f = frame_index(zo, a.P[2], Do) - a.off[2];
      if (f >= 0 && f < Ds) sz = f;
    }
    src_z[t - kTX] = sz;
  }
  __syncthreads();

  const int z = z0 + lane;
  const int sz = src_z[lane];
  const long long zi = (long long)sz * a.is[2], zl = (long long)sz * a.ls[2];
  int mm[6] = {INT_MAX, -1, INT_MAX, -1, INT_MAX, -1};
  for (int xi = wave; xi < kTX; xi += kNT / 64) {
    const long long oi = off_i[xi], ol = off_l[xi];
    float v = 0.f;
    int l = 0;
    if (sz >= 0 && oi != kOutside) {
      v = img[oi + zi];
      l = a.lab_bytes == 1 ? (int)static_cast<const uint8_t*>(lab)[ol + zl] : (static_cast<const int32_t*>(lab)[ol + zl] & 255);
      if (a.normalise) {
        v = __fdiv_rn(__fsub_rn(v, 300.f), -600.f);
        v = v > 1.f ? 1.f : (v < 0.f ? 0.f : v);
      }
    }
    timg[lane * kPitch + xi] = v;
    tlab[lane * kPitch + xi] = l;
    if (l != 0) {
      const int x = x0 + xi;
      mm[0] = z < mm[0] ? z : mm[0]; mm[1] = z > mm[1] ? z : mm[1];
      mm[2] = y; mm[3] = y;
      mm[4] = x < mm[4] ? x : mm[4]; mm[5] = x > mm[5] ? x : mm[5];
    }
  }
  __syncthreads();

  if (vec) {                           // W' % 4 == 0, 16-byte aligned outputs: a quad of x per lane
    const int x4 = (t & 15) * 4;
    if (x0 + x4 < Wo) {
      for (int zz = t >> 4; zz < kTZ; zz += kNT / 16) {
        const int zo = z0 + zz;
        if (zo >= Do) break;
        const long long o = ((long long)zo * Ho + y) * Wo + x0 + x4;
        const float* r = timg + zz * kPitch + x4;
        const int* q = tlab + zz * kPitch + x4;
        *reinterpret_cast<float4*>(oimg + o) = make_float4(r[0], r[1], r[2], r[3]);
        *reinterpret_cast<uint32_t*>(olab + o) = (uint32_t)q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16) | ((uint32_t)q[3] << 24);
      }
    }
  } else if (x0 + lane < Wo) {
    for (int zz = wave; zz < kTZ; zz += kNT / 64) {
      const int zo = z0 + zz;
      if (zo >= Do) break;
      const long long o = ((long long)zo * Ho + y) * Wo + x0 + lane;
      oimg[o] = timg[zz * kPitch + lane];
      olab[o] = (uint8_t)tlab[zz * kPitch + lane];
    }
  }

  const int wg = ((int)blockIdx.z * (int)gridDim.y + (int)blockIdx.y) * (int)gridDim.x + (int)blockIdx.x;
  block_minmax6(mm, partials + (long long)wg * 6);
}

// ------------------------------------------------------------------------------------------------------- RPN targets
struct Box6 { double v[6]; };

__device__ __forceinline__ Box6 load_box(const float* __restrict__ p) {
  Box6 b;
#pragma unroll
  for (int k = 0; k < 6; ++k) b.v[k] = (double)p[k];
  return b;
}
__device__ __forceinline__ double box_volume(const Box6& b) { return (b.v[3] - b.v[0]) * (b.v[4] - b.v[1]) * (b.v[5] - b.v[2]); }
__device__ __forceinline__ double dmax(double a, double b) { return a > b ? a : b; }
__device__ __forceinline__ double dmin(double a, double b) { return a < b ? a : b; }

// utils.compute_iou(gt, anchors, gt_volume, anchor_volumes)[a] in double
__device__ __forceinline__ double iou_of(const Box6& g, double gvol, const Box6& a, double avol) {
  const double z1 = dmax(g.v[0], a.v[0]), z2 = dmin(g.v[3], a.v[3]);
  const double y1 = dmax(g.v[1], a.v[1]), y2 = dmin(g.v[4], a.v[4]);
  const double x1 = dmax(g.v[2], a.v[2]), x2 = dmin(g.v[5], a.v[5]);
  const double inter = dmax(x2 - x1, 0.0) * dmax(y2 - y1, 0.0) * dmax(z2 - z1, 0.0);
  const double uni = gvol + avol - inter;
  return inter / (uni + 1e-6);
}

// (value, index) arg-max with the first index winning a tie, over the workgroup; thread 0 gets the result
__device__ __forceinline__ void block_argmax(double& v, int& i) {
  __shared__ double rv[kNT / 64];
  __shared__ int ri[kNT / 64];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double ov = __shfl_xor(v, o, 64);
    const int oi = __shfl_xor(i, o, 64);
    if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
  }
  __syncthreads();                      // (the previous round's rv / ri have been read)
  if ((threadIdx.x & 63) == 0) { rv[threadIdx.x >> 6] = v; ri[threadIdx.x >> 6] = i; }
  __syncthreads();
  if (threadIdx.x == 0)
    for (int w = 1; w < kNT / 64; ++w)
      if (rv[w] > v || (rv[w] == v && ri[w] < i)) { v = rv[w]; i = ri[w]; }
}

__global__ void __launch_bounds__(kNT)
k_rpn_iou(const float* __restrict__ anchors, int A, const float* __restrict__ gt, int G, double* __restrict__ iou_max,
          int32_t* __restrict__ iou_arg, double* __restrict__ part_v, int32_t* __restrict__ part_i) {
  const int a = blockIdx.x * kNT + threadIdx.x;
  const bool valid = a < A;
  Box6 ab = {};
  double avol = 0.0;
  if (valid) { ab = load_box(anchors + (long long)a * 6); avol = box_volume(ab); }
  double best = 0.0;
  int arg = 0;
  for (int g = 0; g < G; ++g) {
    const Box6 gb = load_box(gt + g * 6);
    const double iou = iou_of(gb, box_volume(gb), ab, avol);
    if (g == 0 || iou > best) { best = iou; arg = g; }        // np.argmax(overlaps, axis = 1): the first maximum
    double v = valid ? iou : -INFINITY;
    int i = valid ? a : INT_MAX;
    block_argmax(v, i);
    if (threadIdx.x == 0) { part_v[(long long)blockIdx.x * G + g] = v; part_i[(long long)blockIdx.x * G + g] = i; }
  }
  if (valid) { iou_max[a] = best; iou_arg[a] = arg; }
}

__global__ void __launch_bounds__(kNT)
k_rpn_gt_best(const double* __restrict__ part_v, const int32_t* __restrict__ part_i, int nwg, int G, int32_t* __restrict__ gt_best) {
  for (int g = 0; g < G; ++g) {
    double v = -INFINITY;
    int i = INT_MAX;
    for (int w = threadIdx.x; w < nwg; w += kNT) {
      const double ov = part_v[(long long)w * G + g];
      const int oi = part_i[(long long)w * G + g];
      if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
    }
    block_argmax(v, i);
    if (threadIdx.x == 0) gt_best[g] = i;
  }
}

__global__ void __launch_bounds__(kNT)
k_rpn_match(const double* __restrict__ iou_max, const int32_t* __restrict__ gt_best, int A, int G, double neg_iou, double pos_iou,
            int32_t* __restrict__ match) {
  const int a = blockIdx.x * kNT + threadIdx.x;
  if (a >= A) return;
  const double m = iou_max[a];
  int r = m < neg_iou ? -1 : 0;
  for (int g = 0; g < G; ++g)
    if (gt_best[g] == a) r = 1;
  if (m >= pos_iou) r = 1;
  match[a] = r;
}

struct SelectArgs {
  double std_dev[6];
  int A, G, R;
};

// Of the anchors with match == cls keep the K smallest in (key, index) order, set the others neutral; returns the number kept.
// One workgroup; an 8-bit radix select over the 64-bit composite key << 32 | index (unique, so the K-th smallest is a threshold).
__device__ int select_smallest(int32_t* match, const uint32_t* __restrict__ keys, int A, int cls, int K) {
  __shared__ int hist[256];
  __shared__ int sh_n, sh_digit, sh_rem;
  const int t = threadIdx.x, lane = t & 63;
  if (t == 0) sh_n = 0;
  __syncthreads();
  int mine = 0;
  for (int i = t; i < A; i += kNT) mine += match[i] == cls;
  if (mine) atomicAdd(&sh_n, mine);
  __syncthreads();
  const int n = sh_n;
  __syncthreads();
  if (n <= K) return n;
  if (K <= 0) {
    for (int i = t; i < A; i += kNT)
      if (match[i] == cls) match[i] = 0;
    return 0;
  }
  unsigned long long prefix = 0, mask = 0;
  int rem = K;                                   // 1-based rank of the target among the candidates that share the prefix
  for (int b = 7; b >= 0; --b) {
    if (b < 4 && (unsigned long long)A <= (1ull << (8 * b))) continue;      // index bytes that are zero for every anchor
    hist[t] = 0;                                 // (kNT == 256 bins)
    __syncthreads();
    for (int i = t; i < A; i += kNT) {
      if (match[i] != cls) continue;
      const unsigned long long comp = ((unsigned long long)keys[i] << 32) | (unsigned)i;
      if ((comp & mask) == prefix) atomicAdd(&hist[(int)((comp >> (8 * b)) & 255)], 1);
    }
    __syncthreads();
    if (t < 64) {                                // wave 0: inclusive scan of the 256 bins, 4 per lane
      const int h0 = hist[4 * lane], h1 = hist[4 * lane + 1], h2 = hist[4 * lane + 2], h3 = hist[4 * lane + 3];
      int incl = h0 + h1 + h2 + h3;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const int up = __shfl(incl, lane >= o ? lane - o : lane, 64);
        if (lane >= o) incl += up;
      }
      const int excl = incl - (h0 + h1 + h2 + h3);
      if (excl < rem && rem <= incl) {           // exactly one lane
        int d = 0, c = excl;
        if (c + h0 < rem) { c += h0; d = 1;
          if (c + h1 < rem) { c += h1; d = 2;
            if (c + h2 < rem) { c += h2; d = 3; } } }
        sh_digit = 4 * lane + d;
        sh_rem = rem - c;
      }
    }
    __syncthreads();
    prefix |= (unsigned long long)sh_digit << (8 * b);
    mask |= 255ull << (8 * b);
    rem = sh_rem;
    __syncthreads();
  }
  for (int i = t; i < A; i += kNT) {
    if (match[i] != cls) continue;
    const unsigned long long comp = ((unsigned long long)keys[i] << 32) | (unsigned)i;
    if (comp > prefix) match[i] = 0;
  }
  return K;
}

__global__ void __launch_bounds__(kNT)
k_rpn_select(int32_t* match, const uint32_t* __restrict__ keys, const float* __restrict__ anchors, const float* __restrict__ gt,
             const int32_t* __restrict__ iou_arg, float* __restrict__ rpn_bbox, int32_t* __restrict__ counts, SelectArgs s) {
  __shared__ int cnt[kNT];
  const int t = threadIdx.x;
  const int pos = select_smallest(match, keys, s.A, 1, s.R / 2);
  __syncthreads();
  const int neg = select_smallest(match, keys, s.A, -1, s.R - pos);
  __syncthreads();
  if (t == 0) { counts[0] = pos; counts[1] = neg; }

  // the kept positives in ascending anchor order: each thread owns a contiguous run of anchors
  const int chunk = (s.A + kNT - 1) / kNT;
  const int lo = t * chunk < s.A ? t * chunk : s.A, hi = lo + chunk < s.A ? lo + chunk : s.A;
  int c = 0;
  for (int i = lo; i < hi; ++i) c += match[i] == 1;
  cnt[t] = c;
  __syncthreads();
  int row = 0;
  for (int k = 0; k < t; ++k) row += cnt[k];
  for (int i = lo; i < hi; ++i) {
    if (match[i] != 1) continue;
    if (row < s.R) {
      const Box6 a = load_box(anchors + (long long)i * 6), g = load_box(gt + iou_arg[i] * 6);
      float* out = rpn_bbox + (long long)row * 6;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const double gs = g.v[k + 3] - g.v[k], as = a.v[k + 3] - a.v[k];
        const double gc = g.v[k] + 0.5 * gs, ac = a.v[k] + 0.5 * as;
        out[k] = (float)((gc - ac) / as / s.std_dev[k]);
        out[k + 3] = (float)(log(gs / as) / s.std_dev[k + 3]);
      }
    }
    ++row;
  }
  for (int i = pos * 6 + t; i < s.R * 6; i += kNT) rpn_bbox[i] = 0.f;
}

struct RpnLayout { size_t iou_max, iou_arg, part_v, part_i, gt_best, total; int nwg; };

RpnLayout rpn_layout(int A, int G) {
  RpnLayout l;
  l.nwg = (A + kNT - 1) / kNT;
  size_t o = 0;
  l.iou_max = o; o = cfun_align_up(o + (size_t)A * sizeof(double), 16);
  l.part_v = o;  o = cfun_align_up(o + (size_t)l.nwg * G * sizeof(double), 16);
  l.iou_arg = o; o = cfun_align_up(o + (size_t)A * sizeof(int32_t), 16);
  l.part_i = o;  o = cfun_align_up(o + (size_t)l.nwg * G * sizeof(int32_t), 16);
  l.gt_best = o; o = cfun_align_up(o + (size_t)G * sizeof(int32_t), 16);
  l.total = o;
  return l;
}

size_t rotate_workgroups(int H, int W, int D) {
  return (size_t)((W + kTX - 1) / kTX) * (size_t)H * (size_t)((D + kTZ - 1) / kTZ);
}

}  // namespace

extern "C" size_t cfun_sample_workspace_bytes(int32_t H, int32_t W, int32_t D, int32_t A, int32_t G) {
  size_t rot = 0, rpn = 0;
  if (H > 0 && W > 0 && D > 0) rot = rotate_workgroups(H, W, D) * 6 * sizeof(int32_t);
  if (A > 0 && G > 0) rpn = rpn_layout(A, G).total;
  return rot > rpn ? rot : rpn;
}

extern "C" int cfun_sample_rotate_bbox(const float* image, const int64_t* image_strides, const int32_t* label,
                                       const int64_t* label_strides, const int32_t* dims, double cos_t, double sin_t,
                                       int32_t rotate, float* out_image, uint8_t* out_label, int32_t* raw_box, int32_t* box,
                                       int32_t* empty, void* workspace, size_t workspace_bytes, cfun_stream_t stream) {
  if (!image || !label || !image_strides || !label_strides || !dims || !out_image || !out_label || !raw_box || !box || !empty)
    return CFUN_EINVAL;
  RotArgs a;
  a.H = dims[0]; a.W = dims[1]; a.D = dims[2];
  if (a.H <= 0 || a.W <= 0 || a.D <= 0 || a.H > 65535) return CFUN_EINVAL;
  for (int d = 0; d < 3; ++d) { a.is[d] = image_strides[d]; a.ls[d] = label_strides[d]; }
  a.c = cos_t; a.s = sin_t; a.rotate = rotate;
  const size_t nwg = rotate_workgroups(a.H, a.W, a.D);
  if ((size_t)((a.D + kTZ - 1) / kTZ) > 65535 || nwg > (size_t)INT_MAX / 6) return CFUN_EINVAL;
  if (!workspace || workspace_bytes < nwg * 6 * sizeof(int32_t)) return CFUN_EWORKSPACE;
  int32_t* partials = (int32_t*)workspace;
  const int vec = (a.W % 4 == 0) && cfun_aligned16(out_image) && (((uintptr_t)out_label) & 3) == 0;
  hipLaunchKernelGGL(k_rotate_relay, dim3((unsigned)((a.W + kTX - 1) / kTX), (unsigned)a.H, (unsigned)((a.D + kTZ - 1) / kTZ)),
                     dim3(kNT), 0, cfun_st(stream), image, label, out_image, out_label, partials, a, vec);
  CFUN_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_box_finish, dim3(1), dim3(kNT), 0, cfun_st(stream), (const int32_t*)partials, (int)nwg, a.H, a.W, a.D,
                     raw_box, box, empty);
  CFUN_LAUNCH_CHECK();
  return CFUN_OK;
}

extern "C" int cfun_sample_rpn_targets(const float* anchors, int32_t A, const float* gt_boxes, int32_t G, const uint32_t* keys,
                                       int32_t R, const double* std_dev, double neg_iou, double pos_iou, int32_t* rpn_match,
                                       float* rpn_bbox, int32_t* counts, void* workspace, size_t workspace_bytes,
                                       cfun_stream_t stream) {
  if (A < 0 || G < 0 || R < 0 || !std_dev) return CFUN_EINVAL;
  if (A == 0 || G == 0) return CFUN_OK;
  if (!anchors || !gt_boxes || !keys || !rpn_match || !counts || (R > 0 && !rpn_bbox)) return CFUN_EINVAL;
  const RpnLayout l = rpn_layout(A, G);
  if (!workspace || workspace_bytes < l.total) return CFUN_EWORKSPACE;
  char* ws = (char*)workspace;
  double* iou_max = (double*)(ws + l.iou_max);
  int32_t* iou_arg = (int32_t*)(ws + l.iou_arg);
  double* part_v = (double*)(ws + l.part_v);
  int32_t* part_i = (int32_t*)(ws + l.part_i);
  int32_t* gt_best = (int32_t*)(ws + l.gt_best);
  SelectArgs s;
  for (int k = 0; k < 6; ++k) s.std_dev[k] = std_dev[k];
  s.A = A; s.G = G; s.R = R;
  hipStream_t st = cfun_st(stream);
  hipLaunchKernelGGL(k_rpn_iou, dim3((unsigned)l.nwg), dim3(kNT), 0, st, anchors, (int)A, gt_boxes, (int)G, iou_max, iou_arg, part_v,
                     part_i);
  CFUN_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_rpn_gt_best, dim3(1), dim3(kNT), 0, st, (const double*)part_v, (const int32_t*)part_i, l.nwg, (int)G, gt_best);
  CFUN_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_rpn_match, dim3((unsigned)l.nwg), dim3(kNT), 0, st, (const double*)iou_max, (const int32_t*)gt_best, (int)A,
                     (int)G, neg_iou, pos_iou, rpn_match);
  CFUN_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_rpn_select, dim3(1), dim3(kNT), 0, st, rpn_match, keys, anchors, gt_boxes, (const int32_t*)iou_arg, rpn_bbox,
                     counts, s);
  CFUN_LAUNCH_CHECK();
  return CFUN_OK;
}

extern "C" size_t cfun_sample_lits_workspace_bytes(const int32_t* out_dims) {
  if (!out_dims || out_dims[0] <= 0 || out_dims[1] <= 0 || out_dims[2] <= 0) return 0;
  return rotate_workgroups(out_dims[0], out_dims[1], out_dims[2]) * 6 * sizeof(int32_t);
}

extern "C" int cfun_sample_lits(const float* image, const int64_t* image_strides, const void* label, const int64_t* label_strides,
                                int32_t label_elem_size, const int32_t* dims, const int32_t* frame, const int32_t* offset,
                                const int32_t* out_dims, const double* map, int32_t normalise, float* out_image,
                                uint8_t* out_label, int32_t* raw_box, int32_t* box, int32_t* empty, void* workspace,
                                size_t workspace_bytes, cfun_stream_t stream) {
  if (!image || !label || !image_strides || !label_strides || !dims || !frame || !offset || !out_dims || !out_image ||
      !out_label || !raw_box || !box || !empty)
    return CFUN_EINVAL;
  if (label_elem_size != 1 && label_elem_size != 4) return CFUN_EINVAL;
  LitsArgs a;
  for (int d = 0; d < 3; ++d) {
    a.is[d] = image_strides[d]; a.ls[d] = label_strides[d];
    a.n[d] = dims[d]; a.P[d] = frame[d]; a.off[d] = offset[d]; a.m[d] = out_dims[d];
    if (a.n[d] <= 0 || a.P[d] <= 0 || a.m[d] <= 0 || a.off[d] < 0 || (int64_t)a.off[d] + a.n[d] > (int64_t)a.P[d]) return CFUN_EINVAL;
  }
  a.has_map = map != nullptr;
  for (int k = 0; k < 6; ++k) {
    a.map[k] = map ? map[k] : 0.0;
    if (!isfinite(a.map[k])) return CFUN_EINVAL;
  }
  a.normalise = normalise != 0;
  a.lab_bytes = label_elem_size;
  const int Ho = a.m[0], Wo = a.m[1], Do = a.m[2];
  const size_t nwg = rotate_workgroups(Ho, Wo, Do);
  if (Ho > 65535 || (size_t)((Do + kTZ - 1) / kTZ) > 65535 || nwg > (size_t)INT_MAX / 6) return CFUN_EINVAL;
  if (!workspace || workspace_bytes < nwg * 6 * sizeof(int32_t)) return CFUN_EWORKSPACE;
  int32_t* partials = (int32_t*)workspace;
  const int vec = (Wo % 4 == 0) && cfun_aligned16(out_image) && (((uintptr_t)out_label) & 3) == 0;
  hipLaunchKernelGGL(k_lits_gather, dim3((unsigned)((Wo + kTX - 1) / kTX), (unsigned)Ho, (unsigned)((Do + kTZ - 1) / kTZ)), dim3(kNT),
                     0, cfun_st(stream), image, label, out_image, out_label, partials, a, vec);
  CFUN_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_box_finish, dim3(1), dim3(kNT), 0, cfun_st(stream), (const int32_t*)partials, (int)nwg, Ho, Wo, Do, raw_box,
                     box, empty);
  CFUN_LAUNCH_CHECK();
  return CFUN_OK;
}
