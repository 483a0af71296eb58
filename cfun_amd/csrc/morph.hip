// Ball morphology of a class map on the device (include/cfun_morph.h): erode, dilate, open, close with the ball of a physical
// radius under anisotropic spacing.  Morphology with a ball is a threshold on surface.hip's squared distance field -- "is there a
// seed within r" -- and because the radius is known, this is a BOUNDED transform: bytes in, bytes out, no float field in memory.
// Built with -ffp-contract=off: every comparison below is defined float32 operation by float32 operation.
//
// With tx(k) = fl(float(k * k) * sx2) (ty, tz likewise) and Rx the largest k with tx(k) <= r2 (Ry, Rz likewise; on the host):
//   (a) k_morph_x   x: a workgroup stages a slab of whole rows (consecutive in memory) in LDS as seed bits, formed from the class
//                   map itself (pred == k, its negation, != 0) or from the first half's result; every thread owns one voxel at a
//                   time and scans outwards for the index distance kx to the row's nearest seed, Rx steps at most.  A virtual
//                   seed (outside = 0) is a minimum with min(x + 1, W - x).  Out: kx, or kInf when kx > Rx (tx(kx) > r2 can never
//                   come back under r2: the later sweeps only add non-negative terms).  Not launched when Rx == 0: (b) then
//                   forms kx = 0 / kInf from the seed predicate itself.
//   (b) k_morph_y   y: a slab of whole y lines of one z plane, x-contiguous in LDS and in memory, in place.  Every thread owns one
//                   voxel and takes g2 = min over |dy| <= Ry of fl(tx(kx[y + dy]) + ty(|dy|)) in a register -- the very
//                   operations of the definition -- stopping once ty(|dy|) >= the best so far.  Out: c = 0 when g2 > r2, else
//                   1 + the largest dz with fl(g2 + tz(dz)) <= r2 (a bisection over 0 .. min(Rz, D - 1); the predicate is
//                   monotone in dz).  c says everything the z sweep will ask of g2: a seed cell at distance k along z covers a
//                   voxel iff k < c.  When Rz == 0 the z sweep is the identity; it is not launched and (b) does (d) itself.
//   (c) k_morph_z   z: the same slabs along z; a voxel is covered iff some cell of its line at distance k has c > k, k <= Rz.
//   (d) finish()    the covered bit against the class map: the first half of an open or a close writes its result as a byte
//                   mask into the workspace (the seed set of the second half); the last half writes out and counts.  Counts
//                   go through LDS to one integer atomicAdd per workgroup and field on stats.
// kx and c are index distances: uint8 when min(Rx, W) and min(Rz, D) are at most 254, uint16 otherwise (a radius of hundreds of
// voxels).  They reproduce the float32 comparisons bit for bit because tx, ty, tz are recomputed from them, never stored rounded.
// A slab with no finite cell skips its scans.
//
// Several groups: a loop on the one stream, highest class first, sharing the workspace.  The first group's last kernel copies
// every byte it does not change; later groups only touch their own voxels, and a set reads out for a higher group's claim (those
// launches came before it on the stream), as fill.hip does.  No thread waits for a value another workgroup writes, and every loop
// is bounded by a line length, a reach or a grid stride.
#include "common.h"
#include "../../include/cfun_morph.h"

namespace {

constexpr int kNT = 256;
constexpr int kMaxDim = 4096;                         // float(k * k) is exact below 2^24
constexpr int kSlabBytes = 32768;                     // a sweep's slab: 32 KiB of LDS, 4 or 5 workgroups per CU
constexpr int kMaxLines = 128;                        // y and z sweeps: columns per slab at most (two waves across x)
constexpr int kFields = 2;                            // per group: voxels cleared, voxels set

static_assert(kSlabBytes >= 2 * kMaxDim, "a slab holds at least one whole line of uint16");

enum Fin { kMaskErode = 0, kMaskDilate, kClearCovered, kClearUncovered, kSetCovered, kSetMaskedUncovered };

template <typename T> struct Cell;
template <> struct Cell<uint8_t> { static constexpr int kInf = 0xff; };
template <> struct Cell<uint16_t> { static constexpr int kInf = 0xffff; };

__device__ __forceinline__ float inf32() { return __builtin_huge_valf(); }

struct Seed {
  const uint8_t* src;        // the class map, or the first half's mask
  int val, inv;              // a seed: (src[i] == val) != inv
};
__device__ __forceinline__ bool is_seed(const Seed& s, long long i) { return (s.src[i] == s.val) != (s.inv != 0); }

struct Geo {
  int D, H, W;
  int lines;                 // lines per slab: rows (x sweep) or columns (y and z sweeps)
  int tiles_x;               // y and z sweeps: slabs along x
  int rx, ry, rz;            // the reaches, capped at the line: min(Rx, W), min(Ry, H - 1), min(Rz, D - 1)
  int virt;                  // two virtual seeds per line, at -1 and L
  float sx2, sy2, sz2, r2;
};

struct FinArgs {
  const uint8_t* pred;
  const uint8_t* mask_in;    // kSetMaskedUncovered: the dilation
  uint8_t* mask_out;         // kMaskErode, kMaskDilate
  uint8_t* out;
  unsigned long long* stat;  // the group's row of stats
  int fin, object, value, first;                      // object: the class, or -1 for the foreground
};

// (d) one voxel.  cleared / set: this thread's counts.
__device__ __forceinline__ void finish(bool covered, long long i, const FinArgs& f, unsigned& cleared, unsigned& set) {
  const int c = f.pred[i];
  const bool obj = f.object < 0 ? c != 0 : c == f.object;
  if (f.fin == kMaskErode) { f.mask_out[i] = obj && !covered ? 1 : 0; return; }
  if (f.fin == kMaskDilate) { f.mask_out[i] = covered ? 1 : 0; return; }
  bool clear = false, put = false;
  if (f.fin == kClearCovered) clear = obj && covered;
  else if (f.fin == kClearUncovered) clear = obj && !covered;
  else if (f.fin == kSetCovered) put = c == 0 && covered;
  else put = c == 0 && !covered && f.mask_in[i] != 0;
  if (put) put = f.first || f.out[i] == 0;            // a higher group's claim stands
  if (clear) { f.out[i] = 0; ++cleared; }
  else if (put) { f.out[i] = (uint8_t)f.value; ++set; }
  else if (f.first) f.out[i] = (uint8_t)c;
}

// the workgroup's counts: LDS, then one atomicAdd per field that is not zero.  Sums of integers: the order does not matter.
__device__ __forceinline__ void flush_counts(unsigned long long* acc, unsigned cleared, unsigned set, const FinArgs& f) {
  if (cleared) atomicAdd(&acc[0], (unsigned long long)cleared);
  if (set) atomicAdd(&acc[1], (unsigned long long)set);
  __syncthreads();
  if (threadIdx.x < kFields && acc[threadIdx.x] != 0) atomicAdd(&f.stat[threadIdx.x], acc[threadIdx.x]);
}

// (a) the slab is `lines` whole rows, consecutive in memory: one contiguous stretch of the map
template <typename T>
__global__ void __launch_bounds__(kNT)
k_morph_x(Seed s, T* __restrict__ kx, Geo a) {
  __shared__ uint8_t g[kSlabBytes];
  const int t = threadIdx.x, W = a.W;
  const long long rows = (long long)a.D * a.H, r0 = (long long)blockIdx.x * a.lines;
  const int nl = rows - r0 < a.lines ? (int)(rows - r0) : a.lines;
  const long long base = r0 * W;
  const int cnt = nl * W;                                                      // <= kSlabBytes
  for (int o = t; o < cnt; o += kNT) g[o] = is_seed(s, base + o) ? 1 : 0;
  __syncthreads();
  for (int o = t; o < cnt; o += kNT) {
    const int row = o / W, p = o - row * W;
    const uint8_t* r = g + row * W;
    int found = Cell<T>::kInf;
    for (int k = 0; k <= a.rx; ++k)
      if ((p - k >= 0 && r[p - k]) || (p + k < W && r[p + k])) { found = k; break; }
    if (a.virt) {
      const int kv = p + 1 < W - p ? p + 1 : W - p;
      if (kv <= a.rx && kv < found) found = kv;
    }
    kx[base + o] = (T)found;
  }
}

// (b) the slab is [H][nl], column fastest: consecutive threads hold consecutive addresses, in LDS and in memory
template <typename T>
__global__ void __launch_bounds__(kNT)
k_morph_y(Seed s, int from_seed, T* buf, Geo a, FinArgs f, int last) {
  __shared__ T g[kSlabBytes / sizeof(T)];
  __shared__ unsigned long long acc[kFields];
  __shared__ int any;
  const int t = threadIdx.x, L = a.H;
  const int tx = blockIdx.x % a.tiles_x, z = blockIdx.x / a.tiles_x;
  const int x0 = tx * a.lines;
  const int nl = a.W - x0 < a.lines ? a.W - x0 : a.lines;
  const long long base = (long long)z * a.H * a.W + x0;
  const int cnt = nl * L;                                                      // <= kSlabBytes / sizeof(T)
  if (t == 0) any = 0;
  if (t < kFields) acc[t] = 0;
  __syncthreads();
  bool mine = false;
  for (int o = t; o < cnt; o += kNT) {
    const int p = o / nl, c = o - p * nl;
    const long long i = base + (long long)p * a.W + c;
    const int v = from_seed ? (is_seed(s, i) ? 0 : Cell<T>::kInf) : (int)buf[i];
    g[o] = (T)v;
    mine = mine || v != Cell<T>::kInf;
  }
  if (mine) any = 1;                                                           // (every writer stores the same value)
  __syncthreads();
  const bool scan = any != 0;
  unsigned cleared = 0, set = 0;
  for (int o = t; o < cnt; o += kNT) {
    const int p = o / nl, c = o - p * nl;
    const long long i = base + (long long)p * a.W + c;
    float best = inf32();
    if (scan) {
      const int own = g[o];
      if (own != Cell<T>::kInf) best = (float)(own * own) * a.sx2;
      for (int k = 1; k <= a.ry; ++k) {
        const float tk = (float)(k * k) * a.sy2;
        if (tk >= best) break;                                                 // every later candidate is at least tk
        if (p - k >= 0) {
          const int q = g[o - k * nl];
          if (q != Cell<T>::kInf) {
            const float cand = (float)(q * q) * a.sx2 + tk;
            best = cand < best ? cand : best;
          }
        }
        if (p + k < L) {
          const int q = g[o + k * nl];
          if (q != Cell<T>::kInf) {
            const float cand = (float)(q * q) * a.sx2 + tk;
            best = cand < best ? cand : best;
          }
        }
      }
    }
    if (a.virt) {
      const int kv = p + 1 < L - p ? p + 1 : L - p;
      const float tv = (float)(kv * kv) * a.sy2;
      best = tv < best ? tv : best;
    }
    if (last) {
      finish(best <= a.r2, i, f, cleared, set);
    } else {
      int reach = 0;
      if (best <= a.r2) {
        int lo = 0, hi = a.rz;
        while (lo < hi) {
          const int mid = (lo + hi + 1) >> 1;
          if (best + (float)(mid * mid) * a.sz2 <= a.r2) lo = mid;
          else hi = mid - 1;
        }
        reach = lo + 1;
      }
      buf[i] = (T)reach;
    }
  }
  if (last) flush_counts(acc, cleared, set, f);
}

// (c) the slab is [D][nl] of one y, column fastest
template <typename T>
__global__ void __launch_bounds__(kNT)
k_morph_z(const T* __restrict__ buf, Geo a, FinArgs f) {
  __shared__ T g[kSlabBytes / sizeof(T)];
  __shared__ unsigned long long acc[kFields];
  __shared__ int any;
  const int t = threadIdx.x, L = a.D;
  const int tx = blockIdx.x % a.tiles_x, y = blockIdx.x / a.tiles_x;
  const int x0 = tx * a.lines;
  const int nl = a.W - x0 < a.lines ? a.W - x0 : a.lines;
  const long long base = (long long)y * a.W + x0, pstride = (long long)a.H * a.W;
  const int cnt = nl * L;
  if (t == 0) any = 0;
  if (t < kFields) acc[t] = 0;
  __syncthreads();
  bool mine = false;
  for (int o = t; o < cnt; o += kNT) {
    const int p = o / nl, c = o - p * nl;
    const T v = buf[base + p * pstride + c];
    g[o] = v;
    mine = mine || v != 0;
  }
  if (mine) any = 1;
  __syncthreads();
  const bool scan = any != 0;
  unsigned cleared = 0, set = 0;
  for (int o = t; o < cnt; o += kNT) {
    const int p = o / nl, c = o - p * nl;
    bool covered = false;
    if (scan)
      for (int k = 0; k <= a.rz; ++k)
        if ((p - k >= 0 && (int)g[o - k * nl] > k) || (p + k < L && (int)g[o + k * nl] > k)) { covered = true; break; }
    if (!covered && a.virt) {
      const int kv = p + 1 < L - p ? p + 1 : L - p;
      covered = (float)(kv * kv) * a.sz2 <= a.r2;
    }
    finish(covered, base + p * pstride + c, f, cleared, set);
  }
  flush_counts(acc, cleared, set, f);
}

// no group at all, or a ball that is the origin alone: the map passes through
__global__ void __launch_bounds__(kNT)
k_morph_copy(const uint8_t* __restrict__ pred, uint8_t* __restrict__ out, int n) {
  const long long i = (long long)blockIdx.x * kNT + threadIdx.x;
  if (i < n) out[i] = pred[i];
}

// ---- host
bool dims_ok(const int32_t* d) {
  if (!d) return false;
  for (int i = 0; i < 3; ++i)
    if (d[i] < 0 || d[i] > kMaxDim) return false;
  return (long long)d[0] * d[1] * d[2] < (1ll << 31) - 1;                      // (<= 2^36: no overflow)
}

bool finite_positive(float v) { return v > 0.f && v < __builtin_huge_valf(); } // (NaN fails the first test)

// the largest k <= kMaxDim with fl(float(k * k) * a2) <= r2: the same two float32 operations as on the device
int reach_of(float a2, float r2) {
  int k = 0;
  while (k < kMaxDim && (float)((k + 1) * (k + 1)) * a2 <= r2) ++k;
  return k;
}

int pow2_floor(int v) {
  int p = 1;
  while (p * 2 <= v) p *= 2;
  return p;
}

// the workspace: cells[n] of uint16 at most | mask[n]
size_t cell_bytes(long long n) { return cfun_align_up((size_t)n * sizeof(uint16_t), 256); }
size_t mask_bytes(long long n) { return cfun_align_up((size_t)n, 256); }

// one bounded transform: the seed set through (a) .. (c), finish() in the last kernel launched
template <typename T>
int enqueue_transform(const Seed& s, void* cells, Geo a, int Rx, int Rz, int virt, const FinArgs& f, hipStream_t st) {
  T* buf = (T*)cells;
  constexpr int kSlabCells = kSlabBytes / (int)sizeof(T);
  a.virt = virt;
  if (Rx > 0) {
    const int fit = kSlabBytes / a.W;
    a.lines = fit < 1 ? 1 : fit;
    a.tiles_x = 1;
    const long long rows = (long long)a.D * a.H;
    hipLaunchKernelGGL(k_morph_x<T>, dim3((unsigned)((rows + a.lines - 1) / a.lines)), dim3(kNT), 0, st, s, buf, a);
    CFUN_LAUNCH_CHECK();
  }
  const int last = Rz == 0 ? 1 : 0;
  int fit = kSlabCells / a.H;
  a.lines = pow2_floor(fit < kMaxLines ? fit : kMaxLines);
  a.tiles_x = (a.W + a.lines - 1) / a.lines;
  hipLaunchKernelGGL(k_morph_y<T>, dim3((unsigned)((long long)a.D * a.tiles_x)), dim3(kNT), 0, st, s, Rx > 0 ? 0 : 1, buf, a, f,
                     last);
  CFUN_LAUNCH_CHECK();
  if (!last) {
    fit = kSlabCells / a.D;
    a.lines = pow2_floor(fit < kMaxLines ? fit : kMaxLines);
    a.tiles_x = (a.W + a.lines - 1) / a.lines;
    hipLaunchKernelGGL(k_morph_z<T>, dim3((unsigned)((long long)a.H * a.tiles_x)), dim3(kNT), 0, st, (const T*)buf, a, f);
    CFUN_LAUNCH_CHECK();
  }
  return CFUN_OK;
}

}  // namespace

extern "C" size_t cfun_morph_workspace_bytes(int32_t D, int32_t H, int32_t W, int32_t K) {
  const int32_t d[3] = {D, H, W};
  if (!dims_ok(d) || K < 1 || K > 15 || D == 0 || H == 0 || W == 0) return 0;
  const long long n = (long long)D * H * W;
  return cell_bytes(n) + mask_bytes(n);
}

extern "C" int cfun_morph_apply(const uint8_t* pred, const int32_t* dims, int32_t K, int32_t mode, int32_t op, uint32_t classes,
                                const float* spacing2, float r2, int32_t outside, int32_t fill_value, uint8_t* out, int64_t* stats,
                                void* workspace, size_t workspace_bytes, cfun_stream_t stream) {
  if (!dims_ok(dims) || !stats || !spacing2 || K < 1 || K > 15) return CFUN_EINVAL;
  if (mode != CFUN_CC_CLASS && mode != CFUN_CC_FOREGROUND) return CFUN_EINVAL;
  if (op < CFUN_MORPH_ERODE || op > CFUN_MORPH_CLOSE) return CFUN_EINVAL;
  const bool fg = mode == CFUN_CC_FOREGROUND;
  if (!fg && ((classes & 1u) || (classes >> K) != 0)) return CFUN_EINVAL;
  for (int i = 0; i < 3; ++i)
    if (!finite_positive(spacing2[i])) return CFUN_EINVAL;
  if (!(r2 >= 0.f) || !(r2 < __builtin_huge_valf())) return CFUN_EINVAL;
  if (outside != 0 && outside != 1) return CFUN_EINVAL;
  const bool sets = op == CFUN_MORPH_DILATE || op == CFUN_MORPH_CLOSE;
  if (fg && sets && (fill_value < 1 || fill_value > 255)) return CFUN_EINVAL;
  hipStream_t st = cfun_st(stream);
  const int D = dims[0], H = dims[1], W = dims[2];
  const size_t stat_bytes = (size_t)K * kFields * sizeof(int64_t);
  if (D == 0 || H == 0 || W == 0) {
    if (hipMemsetAsync(stats, 0, stat_bytes, st) != hipSuccess) return CFUN_EINVAL;
    return CFUN_OK;
  }
  if (!pred || !out) return CFUN_EINVAL;
  const long long n64 = (long long)D * H * W;
  const int n = (int)n64;
  if ((uintptr_t)out < (uintptr_t)pred + (uintptr_t)n && (uintptr_t)pred < (uintptr_t)out + (uintptr_t)n) return CFUN_EINVAL;
  if (!workspace || workspace_bytes < cell_bytes(n64) + mask_bytes(n64)) return CFUN_EWORKSPACE;
  if (hipMemsetAsync(stats, 0, stat_bytes, st) != hipSuccess) return CFUN_EINVAL;
  const int Rz = reach_of(spacing2[0], r2), Ry = reach_of(spacing2[1], r2), Rx = reach_of(spacing2[2], r2);
  // the groups, highest class first
  int groups[16], ng = 0;
  if (fg) groups[ng++] = -1;
  else
    for (int k = K - 1; k >= 1; --k)
      if ((classes >> k) & 1u) groups[ng++] = k;
  if (ng == 0 || (Rx == 0 && Ry == 0 && Rz == 0)) {                           // B is the origin alone: every op is the identity
    hipLaunchKernelGGL(k_morph_copy, dim3((unsigned)((n64 + kNT - 1) / kNT)), dim3(kNT), 0, st, pred, out, n);
    CFUN_LAUNCH_CHECK();
    return CFUN_OK;
  }
  Geo a;
  a.D = D; a.H = H; a.W = W;
  a.lines = 1; a.tiles_x = 1; a.virt = 0;
  a.rx = Rx < W ? Rx : W;
  a.ry = Ry < H - 1 ? Ry : H - 1;
  a.rz = Rz < D - 1 ? Rz : D - 1;
  a.sz2 = spacing2[0]; a.sy2 = spacing2[1]; a.sx2 = spacing2[2]; a.r2 = r2;
  const bool narrow = a.rx <= 254 && (Rz < D ? Rz : D) <= 254;               // kx <= rx and c <= rz + 1 fit a byte beside kInf
  void* cells = workspace;
  uint8_t* mask = (uint8_t*)workspace + cell_bytes(n64);
  const int virt = outside ? 0 : 1;
  for (int gi = 0; gi < ng; ++gi) {
    const int g = groups[gi];
    FinArgs f;
    f.pred = pred; f.mask_in = mask; f.mask_out = mask; f.out = out;
    f.stat = (unsigned long long*)stats + (size_t)(fg ? 0 : g) * kFields;
    f.object = g; f.value = fg ? (int)fill_value : g; f.first = gi == 0 ? 1 : 0;
    // seeds of the object and of its complement, read from the class map
    const Seed object{pred, fg ? 0 : g, fg ? 1 : 0}, complement{pred, fg ? 0 : g, fg ? 0 : 1};
    const Seed mask_set{mask, 0, 1}, mask_clear{mask, 0, 0};
    int rc = CFUN_OK;
    auto run = [&](const Seed& s, int v, int fin) {
      f.fin = fin;
      return narrow ? enqueue_transform<uint8_t>(s, cells, a, Rx, Rz, v, f, st)
                    : enqueue_transform<uint16_t>(s, cells, a, Rx, Rz, v, f, st);
    };
    if (op == CFUN_MORPH_ERODE) {
      rc = run(complement, virt, kClearCovered);
    } else if (op == CFUN_MORPH_DILATE) {
      rc = run(object, 0, kSetCovered);
    } else if (op == CFUN_MORPH_OPEN) {
      rc = run(complement, virt, kMaskErode);
      if (rc == CFUN_OK) rc = run(mask_set, 0, kClearUncovered);
    } else {
      rc = run(object, 0, kMaskDilate);
      if (rc == CFUN_OK) rc = run(mask_clear, virt, kSetMaskedUncovered);
    }
    if (rc != CFUN_OK) return rc;
  }
  return CFUN_OK;
}
