// Heart samples from the loader's grid (include/cfun_sample_heart.h): utils.resize_image (order 1, clip, cast back),
// utils.resize_mask (order 0), load_image_gt's per-slice rotation with the re-layout and the GT box, and mold_image's z-score.
//   (a) k_heart_gather   one gather over the OUTPUT: the rotation's source pixel in the resized grid, eight source taps for the
//                        image and one for the label per voxel, clip, cast, re-layout [H,W,D] -> [D',H',W'], and per-workgroup
//                        partials: min / max of z, y, x over label > 0 and the two double sums of the z-score
//   (b) k_heart_finish   one workgroup: partials -> box, 5 % expansion, empty flag (sample.hip's k_box_finish rule), mean and std
//   (c) k_heart_apply    the flat pass (s - mean) / std in place
// No atomics: every grid-wide result goes through per-workgroup partials summed in a fixed order, so two runs agree bit for
// bit.  Built without FMA contraction: the rule is an exact contract with tests/sample_heart_ref.py (the same double operations
// in the same order); only the ORDER of the two sums is this file's own, and the header bounds what that may change.
//
// Tile of (a): native.hip's.  A workgroup owns 64 output y, 64 output x and kHZ output z.  LANES RUN ALONG y.  The heart's
// NIfTI arrays arrive Fortran-ordered (H fastest) from nifti.load, and the resized grid's iy is the axis that follows H: at
// the angles the loader draws (|angle| <= 20 degrees) neighbouring output y step iy by cos(angle) >= 0.94 and ix by
// sin(angle) <= 0.34, so a wave's 64 taps of one (a, b, c) fall into runs along H -- about n / R * 64 elements long without a
// rotation (1.6 * 64 * 2 B = 205 B of int16 at 512 -> 320), broken into about 64 * sin(angle) + 1 <= 23 shorter runs in
// neighbouring columns with one -- where k_rotate_relay's lanes along z would put every lane into a sector of its own (the
// z stride of a Fortran volume is H * W elements).  Each lane reads its own element directly, as in native.hip.  The same
// kernel serves EVERY stride set -- the reads go through the strides -- but only the Fortran order gets these runs: a
// C-ordered source (D fastest) gives one sector per lane and tap pair, which no assignment of lanes to OUTPUT voxels avoids,
// since the output's fastest axis is then the source's slowest.
// A wave takes one x at a time; new against native.hip is that the H and W entries -- f, w0, w1, tap validity, the label's
// order-0 offsets -- are no longer separable, because (iy, ix) depends on both y and x: each thread computes them per output
// pixel, ONCE for all kHZ planes of the tile, and keeps them in registers; the z entries are computed once per workgroup and
// kept in LDS.  Out-of-source taps are loaded from a clamped (valid) address and dropped by a select, so the eight loads of a
// voxel are unconditional and issue together.  Results leave through [64 y][65] dword LDS tiles, one per plane (pitch 65:
// ds_write_b32 banks are (a / 4) % 32, lane = y -> 32 distinct banks per half-wave); the labels of a pixel's kHZ planes share
// one dword of a tile of their own (byte zz = plane zz).  Rows leave along x, 16 B of image and 4 B of label per lane when
// W' % 4 == 0 (k_rotate_relay's store form), 4 B and 1 B otherwise.
// LDS per workgroup: kHZ * 16640 + 16640 B of tiles + the z entries and the reduction's few words, about 50 KB at kHZ = 2:
// three workgroups (12 waves) per CU.  Measured at 512x512x224 -> 320x320x192, rotated and z-scored:
// kHZ = 1 212.6 us, 2 215.8 us, 3 238.8 us (two workgroups per CU), 4 307.6 us (one): the per-pixel work saved by a deeper
// tile does not pay for the waves it costs.
#include <limits.h>
#include <math.h>

#include "common.h"
#include "../../include/cfun_sample_heart.h"

namespace {

constexpr int kNT = 256;
constexpr int kHY = 64, kHX = 64, kHZ = 2, kHPitch = 65;      // heart tile: lanes along y, a column per x, kHZ planes per workgroup
constexpr int kApplyMaxBlocks = 2048;
static_assert(kHZ >= 1 && kHZ <= 4, "the labels of a pixel's planes share one dword");

// One index r of the resized grid on one axis: step 2 of cfun_sample_heart.h.  k: bit 0 / 1 = tap f / f + 1 inside the source.
// o0 / o1: the taps' element offsets, clamped into the source so that a dropped tap still has an address.
struct AxisTaps {
  long long o0, o1;
  double w0, w1;
  int k;
};

__device__ __forceinline__ AxisTaps axis_taps(int r, int n, double q, long long stride) {
  AxisTaps e;
  const double c = ((double)r + 0.5) * q - 0.5;
  const double f = floor(c);
  e.w1 = c - f;
  e.w0 = 1.0 - e.w1;
  const long long f0 = (long long)f, f1 = f0 + 1;
  const bool in0 = f0 >= 0 && f0 < n, in1 = f1 >= 0 && f1 < n;
  e.k = (in0 ? 1 : 0) | (in1 ? 2 : 0);
  e.o0 = (in0 ? f0 : 0) * stride;
  e.o1 = (in1 ? f1 : 0) * stride;
  return e;
}

// cfun_resize3d's order-0 index (resize.hip), q = (double)n / (double)R
__device__ __forceinline__ int nearest_index(int r, int n, double q) {
  const int k = (int)floor(((double)r + 0.5) * q);
  return k < 0 ? 0 : (k > n - 1 ? n - 1 : k);
}

__device__ __forceinline__ int load_label(const void* __restrict__ p, long long o, int kind) {
  if (kind == CFUN_LABEL_UINT8) return (int)static_cast<const uint8_t*>(p)[o];
  if (kind == CFUN_LABEL_INT8) return (int)static_cast<const int8_t*>(p)[o];
  if (kind == CFUN_LABEL_INT16) return (int)static_cast<const int16_t*>(p)[o];
  return static_cast<const int32_t*>(p)[o];
}

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

// the two sums of the calling workgroup's threads -> out[0..1] (thread 0 writes): lanes by the xor butterfly, waves in order
__device__ __forceinline__ void block_sum2(double s1, double s2, double* __restrict__ out) {
  __shared__ double red[kNT / 64][2];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  s1 = cfun_wave_sum_d(s1);
  s2 = cfun_wave_sum_d(s2);
  if (lane == 0) { red[wave][0] = s1; red[wave][1] = s2; }
  __syncthreads();
  if (threadIdx.x == 0) {
    double a = red[0][0], b = red[0][1];
    for (int w = 1; w < kNT / 64; ++w) { a += red[w][0]; b += red[w][1]; }
    out[0] = a;
    out[1] = b;
  }
}

struct HeartArgs {
  int64_t is[3], ls[3];      // element strides of image / label along H, W, D
  int n[3], m[3];            // source extent H, W, D; output extent H', W', D'
  double q[3];               // (double)n / (double)m per axis
  double c, s;
  int ntx, nty;              // tiles along x and y
  int rotate, truncate, has_clip, has_label, label_kind;
};

struct ZEntry {
  AxisTaps taps;
  long long lab;             // the label's offset along D
  int valid;                 // the plane exists (z < D')
};

template <typename T>
__global__ void __launch_bounds__(kNT)
k_heart_gather(const T* __restrict__ img, const void* __restrict__ lab, float* __restrict__ oimg, uint8_t* __restrict__ olab,
               const double* __restrict__ clip, double* __restrict__ sums, int32_t* __restrict__ boxes, HeartArgs a, int vec) {
  __shared__ float timg[kHZ * kHY * kHPitch];
  __shared__ uint32_t tlab[kHY * kHPitch];
  __shared__ ZEntry ez[kHZ];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int Ho = a.m[0], Wo = a.m[1], Do = a.m[2];
  const int bid = (int)blockIdx.x;
  const int x0 = (bid % a.ntx) * kHX, y0 = ((bid / a.ntx) % a.nty) * kHY, z0 = (bid / (a.ntx * a.nty)) * kHZ;

  if (t < kHZ) {
    const int zo = z0 + t;
    ZEntry e;
    e.valid = zo < Do;
    const int r = e.valid ? zo : 0;
    e.taps = axis_taps(r, a.n[2], a.q[2], a.is[2]);
    e.lab = (long long)nearest_index(r, a.n[2], a.q[2]) * a.ls[2];
    ez[t] = e;
  }
  double lo = 0.0, hi = 0.0;
  if (a.has_clip) { lo = clip[0]; hi = clip[1]; }
  __syncthreads();

  const int y = y0 + lane;
  double s1 = 0.0, s2 = 0.0;
  int mm[6] = {INT_MAX, -1, INT_MAX, -1, INT_MAX, -1};
  for (int xi = wave; xi < kHX; xi += kNT / 64) {
    const int x = x0 + xi;
    // step 1: the pixel of the resized grid this output pixel shows
    double fy = (double)y, fx = (double)x;
    if (a.rotate) {
      const double cy = (double)Ho / 2.0 - 0.5, cx = (double)Wo / 2.0 - 0.5;
      const double dx = (double)x - cx, dy = (double)y - cy;
      const double sx = a.c * dx + a.s * dy + cx;
      const double sy = -a.s * dx + a.c * dy + cy;
      fx = floor(sx + 0.5);
      fy = floor(sy + 0.5);
    }
    const bool in = y < Ho && x < Wo && fx >= 0.0 && fx < (double)Wo && fy >= 0.0 && fy < (double)Ho;
    const int iy = in ? (int)fy : 0, ix = in ? (int)fx : 0;
    // the H and W entries of (iy, ix): once for all planes of the tile
    const AxisTaps my = axis_taps(iy, a.n[0], a.q[0], a.is[0]), mx = axis_taps(ix, a.n[1], a.q[1], a.is[1]);
    const long long lyx = (long long)nearest_index(iy, a.n[0], a.q[0]) * a.ls[0] + (long long)nearest_index(ix, a.n[1], a.q[1]) * a.ls[1];
    const long long oy[2] = {my.o0, my.o1}, ox[2] = {mx.o0, mx.o1};
    const double wy[2] = {my.w0, my.w1}, wx[2] = {mx.w0, mx.w1};
    uint32_t lpack = 0;
#pragma unroll
    for (int zz = 0; zz < kHZ; ++zz) {
      const ZEntry mz = ez[zz];
      float s = 0.f;
      int l = 0;
      if (in && mz.valid) {
        const long long oz[2] = {mz.taps.o0, mz.taps.o1};
        const double wz[2] = {mz.taps.w0, mz.taps.w1};
        double v[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) v[q] = (double)img[oy[q >> 2] + ox[(q >> 1) & 1] + oz[q & 1]];
        if (a.has_label) l = load_label(lab, lyx + mz.lab, a.label_kind);
        double acc = 0.0;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          const int ia = q >> 2, ib = (q >> 1) & 1, ic = q & 1;
          const bool inside = ((my.k >> ia) & (mx.k >> ib) & (mz.taps.k >> ic) & 1) != 0;
          const double term = ((v[q] * wy[ia]) * wx[ib]) * wz[ic];
          acc = inside ? acc + term : acc;
        }
        if (a.has_clip) {
          acc = acc < lo ? lo : acc;
          acc = acc > hi ? hi : acc;
        }
        if (a.truncate) acc = trunc(acc) + 0.0;          // (-0.0 + 0.0 = +0.0: an integer has no negative zero)
        s = (float)acc;
      }
      timg[(zz * kHY + lane) * kHPitch + xi] = s;
      lpack |= (uint32_t)(l & 255) << (8 * zz);
      s1 += (double)s;                                   // (a voxel outside the output or the rotation adds its 0)
      s2 += (double)s * (double)s;
      if (l > 0) {
        const int z = z0 + zz;
        mm[0] = z < mm[0] ? z : mm[0]; mm[1] = z > mm[1] ? z : mm[1];
        mm[2] = y < mm[2] ? y : mm[2]; mm[3] = y > mm[3] ? y : mm[3];
        mm[4] = x < mm[4] ? x : mm[4]; mm[5] = x > mm[5] ? x : mm[5];
      }
    }
    tlab[lane * kHPitch + xi] = lpack;
  }
  __syncthreads();

  for (int zz = 0; zz < kHZ; ++zz) {
    const int zo = z0 + zz;
    if (zo >= Do) break;                                 // (uniform over the workgroup)
    const float* plane = timg + zz * kHY * kHPitch;
    if (vec) {                         // W' % 4 == 0, aligned outputs: a quad of x per lane, 16 rows per step
      const int x4 = (t & 15) * 4;
      if (x0 + x4 < Wo) {
        for (int yy = t >> 4; yy < kHY; yy += kNT / 16) {
          const int yo = y0 + yy;
          if (yo >= Ho) break;
          const long long o = ((long long)zo * Ho + yo) * Wo + x0 + x4;
          const float* r = plane + yy * kHPitch + x4;
          *reinterpret_cast<float4*>(oimg + o) = make_float4(r[0], r[1], r[2], r[3]);
          if (a.has_label) {
            const uint32_t* q = tlab + yy * kHPitch + x4;
            const int sh = 8 * zz;
            *reinterpret_cast<uint32_t*>(olab + o) = ((q[0] >> sh) & 255u) | (((q[1] >> sh) & 255u) << 8) |
                                                     (((q[2] >> sh) & 255u) << 16) | (((q[3] >> sh) & 255u) << 24);
          }
        }
      }
    } else if (x0 + lane < Wo) {
      for (int yy = wave; yy < kHY; yy += kNT / 64) {
        const int yo = y0 + yy;
        if (yo >= Ho) break;
        const long long o = ((long long)zo * Ho + yo) * Wo + x0 + lane;
        oimg[o] = plane[yy * kHPitch + lane];
        if (a.has_label) olab[o] = (uint8_t)(tlab[yy * kHPitch + lane] >> (8 * zz));
      }
    }
  }

  block_sum2(s1, s2, sums + (long long)bid * 2);
  if (a.has_label) block_minmax6(mm, boxes + (long long)bid * 6);
}

__global__ void __launch_bounds__(kNT)
k_heart_finish(const double* __restrict__ sums, const int32_t* __restrict__ boxes, int n, int H, int W, int D, int has_label,
               int zscore, int32_t* __restrict__ raw_box, int32_t* __restrict__ box, int32_t* __restrict__ empty,
               double* __restrict__ stats) {
  __shared__ int total[6];
  __shared__ double sum2[2];
  if (zscore) {
    double s1 = 0.0, s2 = 0.0;
    for (int i = threadIdx.x; i < n; i += kNT) { s1 += sums[(long long)i * 2]; s2 += sums[(long long)i * 2 + 1]; }
    block_sum2(s1, s2, sum2);
    if (threadIdx.x == 0) {
      const double cnt = ((double)D * (double)H) * (double)W;
      const double mean = sum2[0] / cnt;
      const double var = sum2[1] / cnt - mean * mean;
      stats[0] = mean;
      stats[1] = sqrt(var);
    }
  }
  if (!has_label) return;                                // (uniform)
  int mm[6] = {INT_MAX, -1, INT_MAX, -1, INT_MAX, -1};
  for (int i = threadIdx.x; i < n; i += kNT) {
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      const int p = boxes[(long long)i * 6 + k];
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

__global__ void __launch_bounds__(kNT)
k_heart_apply(float* __restrict__ out, const double* __restrict__ stats, long long n, int vec) {
  const double mean = stats[0], sd = stats[1];
  const long long step = (long long)gridDim.x * kNT;
  if (vec) {                                             // n % 4 == 0, 16-byte aligned
    float4* o4 = reinterpret_cast<float4*>(out);
    for (long long i = (long long)blockIdx.x * kNT + threadIdx.x; i < n / 4; i += step) {
      float4 v = o4[i];
      v.x = (float)(((double)v.x - mean) / sd);
      v.y = (float)(((double)v.y - mean) / sd);
      v.z = (float)(((double)v.z - mean) / sd);
      v.w = (float)(((double)v.w - mean) / sd);
      o4[i] = v;
    }
  } else {
    for (long long i = (long long)blockIdx.x * kNT + threadIdx.x; i < n; i += step) out[i] = (float)(((double)out[i] - mean) / sd);
  }
}

// a * b * c workgroups on one grid axis, or -1 when that exceeds 2^31 - 1 (no intermediate product overflows 64 bits)
long long tile_count(int a, int b, int c) {
  const long long ab = (long long)a * b;
  if (ab > (long long)INT_MAX) return -1;
  const long long abc = ab * c;
  return abc > (long long)INT_MAX ? -1 : abc;
}

long long heart_tiles(const int32_t* m) {
  return tile_count((m[1] - 1) / kHX + 1, (m[0] - 1) / kHY + 1, (m[2] - 1) / kHZ + 1);      // (not (W + k - 1) / k: overflow near 2^31)
}

constexpr size_t kPartialBytes = 2 * sizeof(double) + 6 * sizeof(int32_t);      // per workgroup: the sums first (8-byte aligned)

template <typename T>
void launch_gather(const void* img, const void* lab, float* oimg, uint8_t* olab, const double* clip, double* sums, int32_t* boxes,
                   const HeartArgs& a, int vec, long long ntiles, hipStream_t st) {
  hipLaunchKernelGGL(k_heart_gather<T>, dim3((unsigned)ntiles), dim3(kNT), 0, st, static_cast<const T*>(img), lab, oimg, olab, clip,
                     sums, boxes, a, vec);
}

}  // namespace

extern "C" size_t cfun_sample_heart_workspace_bytes(const int32_t* out_dims) {
  if (!out_dims || out_dims[0] <= 0 || out_dims[1] <= 0 || out_dims[2] <= 0) return 0;
  const long long ntiles = heart_tiles(out_dims);
  return ntiles < 0 ? 0 : (size_t)ntiles * kPartialBytes;
}

extern "C" int cfun_sample_heart(const void* image, const int64_t* image_strides, int32_t elem_kind, const void* label,
                                 const int64_t* label_strides, int32_t label_kind, const int32_t* dims, const int32_t* out_dims,
                                 const double* clip, int32_t truncate, double cos_t, double sin_t, int32_t rotate, int32_t zscore,
                                 float* out_image, uint8_t* out_label, int32_t* raw_box, int32_t* box, int32_t* empty, double* stats,
                                 void* workspace, size_t workspace_bytes, cfun_stream_t stream) {
  if (!image || !image_strides || !dims || !out_dims || !out_image) return CFUN_EINVAL;
  if (label && (!label_strides || !out_label || !raw_box || !box || !empty)) return CFUN_EINVAL;
  if (zscore && !stats) return CFUN_EINVAL;
  if (elem_kind != CFUN_ELEM_INT16 && elem_kind != CFUN_ELEM_FLOAT32 && elem_kind != CFUN_ELEM_FLOAT64) return CFUN_EINVAL;
  if (label && (label_kind < CFUN_LABEL_INT8 || label_kind > CFUN_LABEL_INT32)) return CFUN_EINVAL;
  HeartArgs a;
  for (int d = 0; d < 3; ++d) {
    a.n[d] = dims[d]; a.m[d] = out_dims[d];
    if (a.n[d] <= 0 || a.m[d] <= 0) return CFUN_EINVAL;
    a.is[d] = image_strides[d];
    a.ls[d] = label ? label_strides[d] : 0;
    a.q[d] = (double)a.n[d] / (double)a.m[d];
  }
  const int Ho = a.m[0], Wo = a.m[1], Do = a.m[2];
  if (Ho > 65535) return CFUN_EINVAL;
  const long long ntiles = heart_tiles(out_dims);
  if (ntiles < 0) return CFUN_EINVAL;
  if (!workspace || workspace_bytes < (size_t)ntiles * kPartialBytes) return CFUN_EWORKSPACE;
  a.c = cos_t; a.s = sin_t;
  a.ntx = (Wo - 1) / kHX + 1;
  a.nty = (Ho - 1) / kHY + 1;
  a.rotate = rotate != 0; a.truncate = truncate != 0; a.has_clip = clip != nullptr; a.has_label = label != nullptr;
  a.label_kind = label_kind;
  double* sums = (double*)workspace;
  int32_t* boxes = (int32_t*)((char*)workspace + (size_t)ntiles * 2 * sizeof(double));
  const int vec = (Wo % 4 == 0) && cfun_aligned16(out_image) && (!label || (((uintptr_t)out_label) & 3) == 0);
  hipStream_t st = cfun_st(stream);
  if (elem_kind == CFUN_ELEM_INT16) launch_gather<int16_t>(image, label, out_image, out_label, clip, sums, boxes, a, vec, ntiles, st);
  else if (elem_kind == CFUN_ELEM_FLOAT32) launch_gather<float>(image, label, out_image, out_label, clip, sums, boxes, a, vec, ntiles, st);
  else launch_gather<double>(image, label, out_image, out_label, clip, sums, boxes, a, vec, ntiles, st);
  CFUN_LAUNCH_CHECK();
  if (!label && !zscore) return CFUN_OK;
  hipLaunchKernelGGL(k_heart_finish, dim3(1), dim3(kNT), 0, st, (const double*)sums, (const int32_t*)boxes, (int)ntiles, Ho, Wo, Do,
                     (int)a.has_label, (int)(zscore != 0), raw_box, box, empty, stats);
  CFUN_LAUNCH_CHECK();
  if (!zscore) return CFUN_OK;
  const long long total = ((long long)Do * Ho) * Wo;
  const int avec = (total % 4 == 0) && cfun_aligned16(out_image);
  const long long work = avec ? total / 4 : total;
  long long nb = (work - 1) / kNT + 1;
  if (nb > kApplyMaxBlocks) nb = kApplyMaxBlocks;
  hipLaunchKernelGGL(k_heart_apply, dim3((unsigned)nb), dim3(kNT), 0, st, out_image, (const double*)stats, total, avec);
  CFUN_LAUNCH_CHECK();
  return CFUN_OK;
}
