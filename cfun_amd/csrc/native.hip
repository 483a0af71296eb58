// LiTS from the scanner's grid (include/cfun_native.h): the two passes either side of the network.
//   (a) k_mold_native   preprocessing.py's order-1 resample to the mean spacing, the clip, the float32 cast, the zero frame, the
//                       nearest resize and the clamp-normalisation of the fork's mold_inputs as ONE gather over the output:
//                       eight taps per output voxel, neither the resampled volume nor the frame built
//   (b) k_map_tile      order-0 resize of a byte map whose source and output have their unit strides on DIFFERENT axes (the
//                       product use: dense [Dr,Hr,Wr] class map -> Fortran [H,W,D] volume): a byte transpose through LDS
//   (c) k_map_plain     the same rule for any other stride pair, one thread per output byte in the output's own order
// No atomics, no scratch, no workspace; every output element is written by exactly one thread, so two runs agree bit for bit.
// Built without FMA contraction: the rule of cfun_native.h is an exact contract with tests/native_ref.py (the same double
// operations in the same order).
//
// Tile of (a).  A NIfTI volume is Fortran-ordered: H fastest, then W, then D.  The output is [D',H',W'] with W' fastest, so
// the pass transposes in the H-W plane.  A workgroup owns 64 output y, 64 output x and kMZ output z.  LANES RUN ALONG y: the
// taps of neighbouring output y sit (P / m) * (n / R) source elements apart along H -- 1.5 to 2.6 at LiTS shapes, so a wave's
// 64 taps of one (a, b, c) fall into a run of about 100 to 170 source elements (200 to 340 B of int16): a handful of 32-byte
// sectors, most of their bytes used by this or the neighbouring tap.  Each lane reads its own element directly (the argument
// sample.hip makes for k_lits_gather's strided z read: no run buffer whose length would depend on the ratio).  A wave takes
// one x at a time and stores its 64 results as a COLUMN of a [64 y][65] float LDS tile (pitch 65 dwords: ds_write_b32 banks
// are (a / 4) % 32, lane = y -> 32 distinct banks per half-wave); rows of the tile leave along x, 16 B per lane when
// W' % 4 == 0 (k_rotate_relay's store form, with its 2-way conflicted quad reads), 4 B per lane otherwise.
// The per-axis part of the rule -- frame index, in-range test, f, w0, w1, tap validity -- is separable: it is computed once per
// workgroup for its 64 y, 64 x and kMZ z by 132 threads and kept in LDS; a voxel costs 8 loads, 24 multiplies and 8 adds
// in double.  Out-of-source taps are loaded from a clamped (valid) address and dropped by a select, so all eight loads of a
// voxel are unconditional and issue together.  The same kernel serves EVERY stride set -- the reads go through the strides --
// but only the Fortran order gets coalesced runs: a C-ordered source (D fastest) gives one sector per lane, which no
// assignment of lanes to OUTPUT voxels avoids, since the output's fastest axis is then the source's slowest.
//
// Tile of (b): eval.hip's byte tile.  Output axis A has unit stride, source axis B != A has unit stride, C is the third.  A
// workgroup owns 128 a x 128 b at one c.  Pass 1: per a, the wave reads the source row along b -- 128 bytes as two 64-lane byte
// loads, through the per-b index table: a near-contiguous gather, n / m source bytes per output byte -- and stores it as a
// COLUMN of a [128 b][132 B] LDS tile (dword index b * 33 + a / 4: the 64 lanes of a store fall on distinct banks).  Pass 2:
// per b, 32 lanes read the 128 bytes of tile row b as dwords (consecutive: no conflict) and store them along a, 4 B per lane
// when the output's other strides and base allow it, 1 B per lane otherwise.
#include <limits.h>
#include <math.h>

#include "common.h"
#include "../../include/cfun_native.h"

namespace {

constexpr int kNT = 256;
constexpr int kMY = 64, kMX = 64, kMZ = 4, kMPitch = 65;      // mold tile: lanes along y, a column per x, kMZ planes per workgroup
constexpr int kBA = 128, kBB = 128, kBPitch = 132;            // byte tile; 132 / 4 = 33 dwords: odd, a column store is conflict-free

// cfun_resize3d's order-0 index (resize.hip)
__device__ __forceinline__ int frame_index(int o, int P, int m) {
  const int k = (int)floor(((double)o + 0.5) * ((double)P / (double)m));
  return k < 0 ? 0 : (k > P - 1 ? P - 1 : k);
}

// One output index of one axis: steps 1-3 of cfun_native.h.  k: bit 0 = r inside the resampled extent, bit 1 / 2 = tap f / f + 1
// inside the source.  o0 / o1: the taps' element offsets, clamped into the source so that a dropped tap still has an address.
struct AxisEntry {
  long long o0, o1;
  double w0, w1;
  int k;
};

__device__ __forceinline__ AxisEntry axis_entry(int o, int m, int P, int off, int n, int R, long long stride) {
  AxisEntry e = {0, 0, 0.0, 0.0, 0};
  if (o >= m) return e;
  const int r = frame_index(o, P, m) - off;
  if (r < 0 || r >= R) return e;
  const double c = ((double)r + 0.5) * ((double)n / (double)R) - 0.5;
  const double f = floor(c);
  e.w1 = c - f;
  e.w0 = 1.0 - e.w1;
  const long long f0 = (long long)f, f1 = f0 + 1;
  const bool in0 = f0 >= 0 && f0 < n, in1 = f1 >= 0 && f1 < n;
  e.k = 1 | (in0 ? 2 : 0) | (in1 ? 4 : 0);
  e.o0 = (in0 ? f0 : 0) * stride;
  e.o1 = (in1 ? f1 : 0) * stride;
  return e;
}

struct MoldArgs {
  int64_t s[3];              // element strides of the source along H, W, D
  int n[3], R[3], P[3], off[3], m[3];
  int ntx, nty;              // tiles along x and y
  int normalise, has_clip;
};

template <typename T>
__global__ void __launch_bounds__(kNT)
k_mold_native(const T* __restrict__ src, float* __restrict__ out, const double* __restrict__ clip, MoldArgs a, int vec) {
  __shared__ float tile[kMY * kMPitch];
  __shared__ AxisEntry ey[kMY], ex[kMX], ez[kMZ];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int Ho = a.m[0], Wo = a.m[1], Do = a.m[2];
  const int bid = (int)blockIdx.x;
  const int x0 = (bid % a.ntx) * kMX, y0 = ((bid / a.ntx) % a.nty) * kMY, z0 = (bid / (a.ntx * a.nty)) * kMZ;

  if (t < kMY) ey[t] = axis_entry(y0 + t, Ho, a.P[0], a.off[0], a.n[0], a.R[0], a.s[0]);
  else if (t < kMY + kMX) ex[t - kMY] = axis_entry(x0 + (t - kMY), Wo, a.P[1], a.off[1], a.n[1], a.R[1], a.s[1]);
  else if (t < kMY + kMX + kMZ) ez[t - kMY - kMX] = axis_entry(z0 + (t - kMY - kMX), Do, a.P[2], a.off[2], a.n[2], a.R[2], a.s[2]);
  double lo = 0.0, hi = 0.0;
  if (a.has_clip) { lo = clip[0]; hi = clip[1]; }
  __syncthreads();

  const AxisEntry my = ey[lane];
  for (int zz = 0; zz < kMZ; ++zz) {
    const int zo = z0 + zz;
    if (zo >= Do) break;                               // (uniform over the workgroup)
    const AxisEntry mz = ez[zz];
    for (int xi = wave; xi < kMX; xi += kNT / 64) {
      const AxisEntry mx = ex[xi];
      float s = 0.f;
      if (my.k & mx.k & mz.k & 1) {
        const long long oy[2] = {my.o0, my.o1}, ox[2] = {mx.o0, mx.o1}, oz[2] = {mz.o0, mz.o1};
        const double wy[2] = {my.w0, my.w1}, wx[2] = {mx.w0, mx.w1}, wz[2] = {mz.w0, mz.w1};
        double v[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) v[q] = (double)src[oy[q >> 2] + ox[(q >> 1) & 1] + oz[q & 1]];
        double acc = 0.0;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          const int ia = q >> 2, ib = (q >> 1) & 1, ic = q & 1;
          const bool inside = ((my.k >> (1 + ia)) & (mx.k >> (1 + ib)) & (mz.k >> (1 + ic)) & 1) != 0;
          const double term = ((v[q] * wy[ia]) * wx[ib]) * wz[ic];
          acc = inside ? acc + term : acc;
        }
        if (a.has_clip) {
          acc = acc < lo ? lo : acc;
          acc = acc > hi ? hi : acc;
        }
        s = (float)acc;
        if (a.normalise) {
          s = __fdiv_rn(__fsub_rn(s, 300.f), -600.f);
          s = s > 1.f ? 1.f : (s < 0.f ? 0.f : s);
        }
      }
      tile[lane * kMPitch + xi] = s;
    }
    __syncthreads();

    if (vec) {                         // W' % 4 == 0, 16-byte aligned output: a quad of x per lane, 16 rows per step
      const int x4 = (t & 15) * 4;
      if (x0 + x4 < Wo) {
        for (int yy = t >> 4; yy < kMY; yy += kNT / 16) {
          const int yo = y0 + yy;
          if (yo >= Ho) break;
          const float* r = tile + yy * kMPitch + x4;
          *reinterpret_cast<float4*>(out + ((long long)zo * Ho + yo) * Wo + x0 + x4) = make_float4(r[0], r[1], r[2], r[3]);
        }
      }
    } else if (x0 + lane < Wo) {
      for (int yy = wave; yy < kMY; yy += kNT / 64) {
        const int yo = y0 + yy;
        if (yo >= Ho) break;
        out[((long long)zo * Ho + yo) * Wo + x0 + lane] = tile[yy * kMPitch + lane];
      }
    }
    __syncthreads();                   // (the tile has been read before the next plane overwrites it)
  }
}

// ------------------------------------------------------------------------------------------------ the byte map (cfun_map_resize)
struct MapArgs {
  int64_t ss[3], os[3];      // element strides of source / output along the kernel's axes (a, b, c)
  int n[3], m[3];            // source / output extents along them
  int nta, ntb;              // tiles along a and b
};

__global__ void __launch_bounds__(kNT)
k_map_tile(const uint8_t* __restrict__ src, uint8_t* __restrict__ out, MapArgs g, int vec) {
  __shared__ __attribute__((aligned(16))) uint8_t tile[kBB * kBPitch];
  __shared__ long long offa[kBA], offb[kBB];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int bid = (int)blockIdx.x;
  const int a0 = (bid % g.nta) * kBA, b0 = ((bid / g.nta) % g.ntb) * kBB, c = bid / (g.nta * g.ntb);
  const int na = g.m[0] - a0 < kBA ? g.m[0] - a0 : kBA, nb = g.m[1] - b0 < kBB ? g.m[1] - b0 : kBB;     // both >= 1

  // the source offset of every a and b of the tile, once per workgroup; positions past the tile's edge repeat its first entry,
  // so every load below is unconditional and in bounds
  if (t < kBA) offa[t] = (long long)frame_index(a0 + (t < na ? t : 0), g.n[0], g.m[0]) * g.ss[0];
  else offb[t - kBA] = (long long)frame_index(b0 + (t - kBA < nb ? t - kBA : 0), g.n[1], g.m[1]) * g.ss[1];
  const long long offc = (long long)frame_index(c, g.n[2], g.m[2]) * g.ss[2];
  __syncthreads();

  const long long pb0 = offb[lane] + offc, pb1 = offb[lane + 64] + offc;
#pragma unroll 8
  for (int aa = wave; aa < na; aa += kNT / 64) {
    const long long row = offa[aa];
    tile[lane * kBPitch + aa] = src[row + pb0];
    tile[(lane + 64) * kBPitch + aa] = src[row + pb1];
  }
  __syncthreads();

  const int a4 = (t & 31) * 4;
  if (a4 < na) {
    const bool whole = vec && a4 + 4 <= na;
    for (int bb = t >> 5; bb < nb; bb += kNT / 32) {
      uint8_t* o = out + (long long)(a0 + a4) * g.os[0] + (long long)(b0 + bb) * g.os[1] + (long long)c * g.os[2];
      const uint8_t* r = tile + bb * kBPitch + a4;
      if (whole) {
        *reinterpret_cast<uint32_t*>(o) = *reinterpret_cast<const uint32_t*>(r);
      } else {
        const int cnt = na - a4 < 4 ? na - a4 : 4;
        for (int k = 0; k < cnt; ++k) o[(long long)k * g.os[0]] = r[k];
      }
    }
  }
}

__global__ void __launch_bounds__(kNT)
k_map_plain(const uint8_t* __restrict__ src, uint8_t* __restrict__ out, MapArgs g, long long total) {
  const long long i = (long long)blockIdx.x * kNT + threadIdx.x;
  if (i >= total) return;
  const int a = (int)(i % g.m[0]);
  const long long rest = i / g.m[0];
  const int b = (int)(rest % g.m[1]), c = (int)(rest / g.m[1]);
  const long long si = (long long)frame_index(a, g.n[0], g.m[0]) * g.ss[0] + (long long)frame_index(b, g.n[1], g.m[1]) * g.ss[1] +
                       (long long)frame_index(c, g.n[2], g.m[2]) * g.ss[2];
  out[(long long)a * g.os[0] + (long long)b * g.os[1] + (long long)c * g.os[2]] = src[si];
}

// a * b * c workgroups on one grid axis, or -1 when that exceeds 2^31 - 1 (no intermediate product overflows 64 bits)
long long tile_count(int a, int b, int c) {
  const long long ab = (long long)a * b;
  if (ab > (long long)INT_MAX) return -1;
  const long long abc = ab * c;
  return abc > (long long)INT_MAX ? -1 : abc;
}

template <typename T>
int launch_mold(const void* src, float* out, const double* clip, const MoldArgs& a, int vec, long long ntiles, hipStream_t st) {
  hipLaunchKernelGGL(k_mold_native<T>, dim3((unsigned)ntiles), dim3(kNT), 0, st, static_cast<const T*>(src), out, clip, a, vec);
  CFUN_LAUNCH_CHECK();
  return CFUN_OK;
}

}  // namespace

extern "C" int cfun_mold_native(const void* src, const int64_t* src_strides, int32_t elem_kind, const int32_t* dims,
                                const int32_t* resampled, const int32_t* frame, const int32_t* offset, const int32_t* out_dims,
                                const double* clip, int32_t normalise, float* out, cfun_stream_t stream) {
  if (!src || !src_strides || !dims || !resampled || !frame || !offset || !out_dims || !out) return CFUN_EINVAL;
  if (elem_kind != CFUN_ELEM_INT16 && elem_kind != CFUN_ELEM_FLOAT32 && elem_kind != CFUN_ELEM_FLOAT64) return CFUN_EINVAL;
  MoldArgs a;
  for (int d = 0; d < 3; ++d) {
    a.s[d] = src_strides[d];
    a.n[d] = dims[d]; a.R[d] = resampled[d]; a.P[d] = frame[d]; a.off[d] = offset[d]; a.m[d] = out_dims[d];
    if (a.n[d] <= 0 || a.R[d] <= 0 || a.P[d] <= 0 || a.m[d] <= 0 || a.off[d] < 0 || (int64_t)a.off[d] + a.R[d] > (int64_t)a.P[d])
      return CFUN_EINVAL;
  }
  a.normalise = normalise != 0;
  a.has_clip = clip != nullptr;
  const int Ho = a.m[0], Wo = a.m[1], Do = a.m[2];
  a.ntx = (Wo - 1) / kMX + 1;                                         // (not (W + k - 1) / k: the sum overflows near 2^31)
  a.nty = (Ho - 1) / kMY + 1;
  const long long ntiles = tile_count(a.ntx, a.nty, (Do - 1) / kMZ + 1);
  if (ntiles < 0) return CFUN_EINVAL;
  const int vec = (Wo % 4 == 0) && cfun_aligned16(out);
  hipStream_t st = cfun_st(stream);
  if (elem_kind == CFUN_ELEM_INT16) return launch_mold<int16_t>(src, out, clip, a, vec, ntiles, st);
  if (elem_kind == CFUN_ELEM_FLOAT32) return launch_mold<float>(src, out, clip, a, vec, ntiles, st);
  return launch_mold<double>(src, out, clip, a, vec, ntiles, st);
}

extern "C" int cfun_map_resize(const uint8_t* src, const int64_t* src_strides, const int32_t* dims, uint8_t* out,
                               const int64_t* out_strides, const int32_t* out_dims, cfun_stream_t stream) {
  if (!src || !src_strides || !dims || !out || !out_strides || !out_dims) return CFUN_EINVAL;
  for (int d = 0; d < 3; ++d)
    if (dims[d] <= 0 || out_dims[d] <= 0 || out_strides[d] <= 0) return CFUN_EINVAL;
  // the output's axes by ascending stride, axes of extent 1 (whose stride addresses nothing) last
  int ord[3] = {0, 1, 2};
  for (int i = 0; i < 3; ++i)
    for (int j = i + 1; j < 3; ++j) {
      const bool oi = out_dims[ord[i]] == 1, oj = out_dims[ord[j]] == 1;
      if ((oi && !oj) || (oi == oj && out_strides[ord[j]] < out_strides[ord[i]])) { const int s = ord[i]; ord[i] = ord[j]; ord[j] = s; }
    }
  for (int i = 0; i + 1 < 3; ++i) {
    const int p = ord[i], q = ord[i + 1];
    if (out_dims[q] == 1) break;
    if (out_strides[q] / out_dims[p] < out_strides[p]) return CFUN_EINVAL;      // stride[q] < stride[p] * extent[p], overflow-free
  }
  hipStream_t st = cfun_st(stream);
  MapArgs g;
  // tiled: the output's unit-stride axis A (the first of the sorted order when its stride is 1) against a DIFFERENT source axis
  // B of unit stride; both of extent > 1, or there is nothing to transpose
  const int A = ord[0];
  int B = -1;
  for (int d = 0; d < 3; ++d)
    if (d != A && src_strides[d] == 1 && dims[d] > 1 && out_dims[d] > 1 && B < 0) B = d;
  if (out_strides[A] == 1 && out_dims[A] > 1 && B >= 0) {
    const int Cx = 3 - A - B;
    const int ax[3] = {A, B, Cx};
    for (int k = 0; k < 3; ++k) { g.ss[k] = src_strides[ax[k]]; g.os[k] = out_strides[ax[k]]; g.n[k] = dims[ax[k]]; g.m[k] = out_dims[ax[k]]; }
    g.nta = (g.m[0] - 1) / kBA + 1;
    g.ntb = (g.m[1] - 1) / kBB + 1;
    const long long ntiles = tile_count(g.nta, g.ntb, g.m[2]);
    if (ntiles < 0) return CFUN_EINVAL;
    const int vec = (((uintptr_t)out) & 3) == 0 && g.os[1] % 4 == 0 && g.os[2] % 4 == 0;
    hipLaunchKernelGGL(k_map_tile, dim3((unsigned)ntiles), dim3(kNT), 0, st, src, out, g, vec);
    CFUN_LAUNCH_CHECK();
    return CFUN_OK;
  }
  for (int k = 0; k < 3; ++k) { g.ss[k] = src_strides[ord[k]]; g.os[k] = out_strides[ord[k]]; g.n[k] = dims[ord[k]]; g.m[k] = out_dims[ord[k]]; }
  g.nta = g.ntb = 0;
  const long long rows = tile_count(g.m[1], g.m[2], 1);                  // (< 2^31, so rows * m[0] stays far inside 64 bits)
  if (rows < 0) return CFUN_EINVAL;
  const long long total = rows * g.m[0];
  const long long nwg = (total + kNT - 1) / kNT;
  if (nwg > (long long)INT_MAX) return CFUN_EINVAL;
  hipLaunchKernelGGL(k_map_plain, dim3((unsigned)nwg), dim3(kNT), 0, st, src, out, g, total);
  CFUN_LAUNCH_CHECK();
  return CFUN_OK;
}
