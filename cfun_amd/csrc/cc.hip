// Connected components of a class map on the device (include/cfun_cc.h): label, then keep the largest component of each group
// and drop the components below a size.  Integers only; no float, no result that depends on arrival order.
//
// cfun_cc_label
//   (a) k_cc_local    a workgroup owns an 8z x 8y x 64x tile: union-find over the tile in LDS (backward half of the neighbourhood:
//                     3 of 6 or 13 of 26 neighbours, those inside the tile), flattened in LDS; labels[i] = 1 + the global index of
//                     the tile-local root, 0 for a zero voxel
//   (b) k_cc_seam     every voxel on a tile boundary unions itself with its backward neighbours that lie in ANOTHER tile, on the
//                     global labels array
//   (c) k_cc_flatten  labels[i] = 1 + root
// cfun_cc_filter
//   (d) k_cc_size     size[root] for every component: aggregated per tile and per label in an LDS table, one global integer add
//                     per (tile, label) -- never one per voxel
//   (e) k_cc_select   per group: components, voxels, voxels in components >= min_voxels, largest (ties: smaller root): LDS
//       k_cc_finish   atomics per workgroup, uint64 partials per workgroup, one finish workgroup per group (as eval.hip)
//   (f) k_cc_write    out = the byte, or 0
//
// The forest.  Cell i of labels holds 1 + the index of i's parent, and a parent's index is never larger than the child's; a root
// holds 1 + its own index.  Links only ever go from a larger root to a smaller index, so a tree's root is the smallest index in
// it, and once every adjacency has been united the root of a voxel is the smallest index of its component: the canonical label.
// Inside a tile the local order (lz, ly, lx) agrees with the global order (z, y, x), so the LDS pass follows the same rule.
//
// Workgroups talk only through integer atomics on global memory and through kernel boundaries.  No workgroup waits for another:
// there is no flag, no ticket, no spin on a value someone else must write, and every loop below ends by itself (see unite()).
// The atomics, the forest, find() and unite() are in cc_forest.h, which fill.hip shares.
#include "common.h"
#include "cc_forest.h"
#include "../../include/cfun_cc.h"

namespace {

constexpr int kNT = 256;
constexpr int kTZ = 8, kTY = 8, kTX = 64;             // the tile; kTX == the wave's width, kTZ * kTY rows
constexpr int kTile = kTZ * kTY * kTX;                // 4096 voxels: 4 KiB of classes, 16 KiB of parents
constexpr int kRows = kTZ * kTY, kRowsPerThread = kRows / (kNT / kTX);
constexpr int kMaxWG = 1536;                          // select pass: workgroups (as eval.hip: 6 per CU)
constexpr int kGroups = 16;                           // K <= 15
constexpr int kFields = 4;                            // per group: components, voxels, voxels kept by min_voxels, best key

struct CcArgs {
  int D, H, W;
  int ntx, nty;              // tiles along x and y
  int n;                     // D * H * W < 2^31 - 1
  int conn26, foreground;
};

__device__ __forceinline__ bool adjacent(int a, int b, int foreground) { return b != 0 && (foreground || a == b); }

// (a) one workgroup per tile.  Thread t owns column lx = t % 64 of the rows t / 64 + 4 j: a wave reads 64 consecutive bytes.
__global__ void __launch_bounds__(kNT)
k_cc_local(const uint8_t* __restrict__ pred, int* __restrict__ labels, CcArgs a) {
  __shared__ uint8_t cls[kTile];
  __shared__ int par[kTile];
  const int t = threadIdx.x, lx = t & (kTX - 1), r0 = t / kTX;
  const int tx = blockIdx.x % a.ntx, rest = blockIdx.x / a.ntx;
  const int ty = rest % a.nty, tz = rest / a.nty;
  const int x0 = tx * kTX, y0 = ty * kTY, z0 = tz * kTZ;
  const int x = x0 + lx;
#pragma unroll
  for (int j = 0; j < kRowsPerThread; ++j) {
    const int row = r0 + j * (kNT / kTX), ly = row % kTY, lz = row / kTY;
    const int y = y0 + ly, z = z0 + lz;
    const int l = row * kTX + lx;
    const bool in = x < a.W && y < a.H && z < a.D;
    cls[l] = in ? pred[((long long)z * a.H + y) * a.W + x] : (uint8_t)0;
    par[l] = l;
  }
  __syncthreads();
  const LdsForest f{par};
  for (int j = 0; j < kRowsPerThread; ++j) {
    const int row = r0 + j * (kNT / kTX), ly = row % kTY, lz = row / kTY;
    const int l = row * kTX + lx;
    const int c = cls[l];
    if (c == 0) continue;
#pragma unroll
    for (int k = 0; k < 13; ++k) {
      if (!a.conn26 && !is_face(k)) continue;
      int dz, dy, dx;
      backward_offset(k, dz, dy, dx);
      const int nz = lz + dz, ny = ly + dy, nx = lx + dx;
      if (nz < 0 || ny < 0 || ny >= kTY || nx < 0 || nx >= kTX) continue;        // another tile: the seam pass
      const int m = (nz * kTY + ny) * kTX + nx;
      if (adjacent(c, cls[m], a.foreground)) unite(f, l, m);
    }
  }
  __syncthreads();                                    // every link is in: par only gets read from here on
#pragma unroll 4
  for (int j = 0; j < kRowsPerThread; ++j) {
    const int row = r0 + j * (kNT / kTX), ly = row % kTY, lz = row / kTY;
    const int y = y0 + ly, z = z0 + lz;
    const int l = row * kTX + lx;
    if (x >= a.W || y >= a.H || z >= a.D) continue;
    int lab = 0;
    if (cls[l] != 0) {
      const int r = find(f, l);
      const int rx = r % kTX, ry = (r / kTX) % kTY, rz = r / (kTX * kTY);
      lab = (int)(((long long)(z0 + rz) * a.H + (y0 + ry)) * a.W + (x0 + rx)) + 1;
    }
    labels[((long long)z * a.H + y) * a.W + x] = lab;
  }
}

// (b) one thread per voxel; only a voxel on the rim of its tile can have a backward neighbour in another tile
__global__ void __launch_bounds__(kNT)
k_cc_seam(const uint8_t* __restrict__ pred, int* labels, CcArgs a) {
  const long long i64 = (long long)blockIdx.x * kNT + threadIdx.x;
  if (i64 >= a.n) return;
  const int i = (int)i64;
  const int x = i % a.W, yz = i / a.W, y = yz % a.H, z = yz / a.H;
  const int lx = x % kTX, ly = y % kTY, lz = z % kTZ;
  if (lx != 0 && lx != kTX - 1 && ly != 0 && ly != kTY - 1 && lz != 0) return;
  const int c = pred[i];
  if (c == 0) return;
  const GlobalForest f{labels};
#pragma unroll
  for (int k = 0; k < 13; ++k) {
    if (!a.conn26 && !is_face(k)) continue;
    int dz, dy, dx;
    backward_offset(k, dz, dy, dx);
    const int nz = z + dz, ny = y + dy, nx = x + dx;
    if (nz < 0 || ny < 0 || ny >= a.H || nx < 0 || nx >= a.W) continue;
    if (nz / kTZ == z / kTZ && ny / kTY == y / kTY && nx / kTX == x / kTX) continue;        // same tile: done in LDS
    const int m = (nz * a.H + ny) * a.W + nx;
    if (adjacent(c, pred[m], a.foreground)) unite(f, i, m);
  }
}

// (c) in place.  A cell is rewritten with 1 + its root while other threads still walk through it: both the old and the new value
// are ancestors of the cell, so their walks end at the same root (no link is made in this launch: roots stay roots).
__global__ void __launch_bounds__(kNT)
k_cc_flatten(int* labels, int n) {
  const long long i = (long long)blockIdx.x * kNT + threadIdx.x;
  if (i >= n) return;
  const GlobalForest f{labels};
  const int p = f.parent((int)i);
  if (p < 0 || p == (int)i) return;
  labels[i] = find(f, p) + 1;
}

// (d) one workgroup per tile (the tile of (a), but any partition would do).  A thread walks its 16 voxels and adds a whole run of
// equal labels at once (inside an organ every voxel of the tile has the same label) to an open-addressing table in LDS: 4096
// slots for at most 4096 distinct labels, so an insert always finds its key or a free slot.  Then one global add per used slot.
__global__ void __launch_bounds__(kNT)
k_cc_size(const int* __restrict__ labels, int* __restrict__ size, CcArgs a) {
  __shared__ int key[kTile];
  __shared__ int cnt[kTile];
  const int t = threadIdx.x, lx = t & (kTX - 1), r0 = t / kTX;
  const int tx = blockIdx.x % a.ntx, rest = blockIdx.x / a.ntx;
  const int ty = rest % a.nty, tz = rest / a.nty;
  const int x = tx * kTX + lx, y0 = ty * kTY, z0 = tz * kTZ;
  for (int s = t; s < kTile; s += kNT) { key[s] = 0; cnt[s] = 0; }
  __syncthreads();
  int run_key = 0, run_n = 0;
  for (int j = 0; j <= kRowsPerThread; ++j) {
    int lab = 0;
    if (j < kRowsPerThread) {
      const int row = r0 + j * (kNT / kTX), y = y0 + row % kTY, z = z0 + row / kTY;
      if (x < a.W && y < a.H && z < a.D) lab = labels[((long long)z * a.H + y) * a.W + x];
    }
    if (lab == run_key) { ++run_n; continue; }
    if (run_key != 0) {
      // lock-free insert: a slot's key goes from 0 to a label once and never changes again
      unsigned h = ((unsigned)run_key * 2654435761u) >> 20;
      for (;;) {
        int k = cc_load_lds(&key[h]);
        if (k == 0) k = cc_cas(&key[h], 0, run_key);
        if (k == 0 || k == run_key) break;
        h = (h + 1) & (kTile - 1);
      }
      atomicAdd(&cnt[h], run_n);
    }
    run_key = lab;
    run_n = 1;
  }
  __syncthreads();
  for (int s = t; s < kTile; s += kNT)
    if (key[s] != 0) atomicAdd(&size[key[s] - 1], cnt[s]);
}

__device__ __forceinline__ int group_of(int c, int K, int foreground) {      // -1: no group
  if (c == 0) return -1;
  if (foreground) return 0;
  return c < K ? c : -1;
}

// a component's key in the contest for "largest": larger size wins, then the smaller root
__device__ __forceinline__ unsigned long long best_key(int sz, int root) {
  return ((unsigned long long)(unsigned)sz << 32) | (unsigned)(0x7fffffff - root);
}

// (e) a grid-stride sweep over the labels; a root is a voxel whose label is 1 + its own index
__global__ void __launch_bounds__(kNT)
k_cc_select(const uint8_t* __restrict__ pred, const int* __restrict__ labels, const int* __restrict__ size,
            unsigned long long* __restrict__ partials, int n, int K, int foreground, long long min_voxels, int nwg) {
  __shared__ unsigned long long acc[kGroups * kFields];
  const int t = threadIdx.x;
  if (t < kGroups * kFields) acc[t] = 0;
  __syncthreads();
  for (long long i = (long long)blockIdx.x * kNT + t; i < n; i += (long long)nwg * kNT) {
    if (labels[i] != (int)i + 1) continue;
    const int g = group_of(pred[i], K, foreground);
    if (g < 0) continue;
    const int sz = size[i];
    atomicAdd(&acc[g * kFields + 0], 1ull);
    atomicAdd(&acc[g * kFields + 1], (unsigned long long)sz);
    if (sz >= min_voxels) atomicAdd(&acc[g * kFields + 2], (unsigned long long)sz);
    cc_max64(&acc[g * kFields + 3], best_key(sz, (int)i));
  }
  __syncthreads();
  if (t < kGroups * kFields) partials[(long long)t * nwg + blockIdx.x] = acc[t];
}

// one workgroup per group: sums and a max of integers, so the order does not matter
__global__ void __launch_bounds__(kNT)
k_cc_finish(const unsigned long long* __restrict__ partials, int nwg, int largest_only, long long min_voxels,
            int64_t* __restrict__ stats, int* __restrict__ winner) {
  __shared__ unsigned long long red[kNT / 64][kFields];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = blockIdx.x;
  unsigned long long v[kFields] = {0, 0, 0, 0};
  for (int w = threadIdx.x; w < nwg; w += kNT) {
#pragma unroll
    for (int f = 0; f < 3; ++f) v[f] += partials[(long long)(g * kFields + f) * nwg + w];
    const unsigned long long b = partials[(long long)(g * kFields + 3) * nwg + w];
    v[3] = b > v[3] ? b : v[3];
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
    for (int f = 0; f < 3; ++f) v[f] += __shfl_xor(v[f], o, 64);
    const unsigned long long b = __shfl_xor(v[3], o, 64);
    v[3] = b > v[3] ? b : v[3];
  }
  if (lane == 0) {
#pragma unroll
    for (int f = 0; f < kFields; ++f) red[wave][f] = v[f];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long s[kFields] = {0, 0, 0, 0};
    for (int w = 0; w < kNT / 64; ++w) {
      for (int f = 0; f < 3; ++f) s[f] += red[w][f];
      s[3] = red[w][3] > s[3] ? red[w][3] : s[3];
    }
    const long long largest = (long long)(s[3] >> 32);
    const long long kept = largest_only ? (s[0] != 0 && largest >= min_voxels ? largest : 0) : (long long)s[2];
    stats[g * 3 + 0] = (long long)s[0];
    stats[g * 3 + 1] = largest;
    stats[g * 3 + 2] = (long long)s[1] - kept;
    winner[g] = s[0] != 0 ? 0x7fffffff - (int)(unsigned)(s[3] & 0xffffffffu) : -1;
  }
}

// (f)
__global__ void __launch_bounds__(kNT)
k_cc_write(const uint8_t* __restrict__ pred, const int* __restrict__ labels, const int* __restrict__ size,
           const int* __restrict__ winner, uint8_t* __restrict__ out, int n, int K, int foreground, int largest_only,
           long long min_voxels) {
  const long long i = (long long)blockIdx.x * kNT + threadIdx.x;
  if (i >= n) return;
  const int c = pred[i];
  const int g = group_of(c, K, foreground);
  bool keep = true;                                   // background, and a byte >= K in class mode, pass through
  if (g >= 0) {
    const int root = labels[i] - 1;
    keep = size[root] >= min_voxels && (!largest_only || root == winner[g]);
  }
  out[i] = keep ? (uint8_t)c : (uint8_t)0;
}

bool dims_ok(int D, int H, int W) {
  if (D < 0 || H < 0 || W < 0) return false;
  if (D == 0 || H == 0 || W == 0) return true;
  const long long lim = (1ll << 31) - 1, dh = (long long)D * H;        // (dh < 2^62; dh * W only once dh is known to be small)
  return dh < lim && dh * W < lim;
}

long long tiles_of(int D, int H, int W) {
  return (long long)((D + kTZ - 1) / kTZ) * ((H + kTY - 1) / kTY) * ((W + kTX - 1) / kTX);
}

int select_wg(long long n) {
  const long long w = (n + kNT * 16 - 1) / (kNT * 16);
  return (int)(w < kMaxWG ? w : kMaxWG);
}

// the filter's workspace: size[n] | partials[kGroups * kFields][nwg] | winner[kGroups]
size_t size_bytes(long long n) { return cfun_align_up((size_t)n * sizeof(int), 256); }
size_t partial_bytes(long long n) { return (size_t)kGroups * kFields * select_wg(n) * sizeof(unsigned long long); }

CcArgs make_args(int D, int H, int W, int connectivity, int mode) {
  CcArgs a;
  a.D = D; a.H = H; a.W = W;
  a.ntx = (W + kTX - 1) / kTX;
  a.nty = (H + kTY - 1) / kTY;
  a.n = (int)((long long)D * H * W);
  a.conn26 = connectivity == 26;
  a.foreground = mode == CFUN_CC_FOREGROUND;
  return a;
}

}  // namespace

extern "C" size_t cfun_cc_workspace_bytes(int32_t D, int32_t H, int32_t W, int32_t K) {
  if (!dims_ok(D, H, W) || K < 1 || K > 15 || D == 0 || H == 0 || W == 0) return 0;
  const long long n = (long long)D * H * W;
  return size_bytes(n) + partial_bytes(n) + kGroups * sizeof(int);
}

extern "C" int cfun_cc_label(const uint8_t* pred, const int32_t* dims, int32_t connectivity, int32_t mode, int32_t* labels,
                             void* workspace, size_t workspace_bytes, cfun_stream_t stream) {
  (void)workspace; (void)workspace_bytes;
  if (!dims || (connectivity != 6 && connectivity != 26) || (mode != CFUN_CC_CLASS && mode != CFUN_CC_FOREGROUND))
    return CFUN_EINVAL;
  if (!dims_ok(dims[0], dims[1], dims[2])) return CFUN_EINVAL;
  if (dims[0] == 0 || dims[1] == 0 || dims[2] == 0) return CFUN_OK;
  if (!pred || !labels) return CFUN_EINVAL;
  const CcArgs a = make_args(dims[0], dims[1], dims[2], connectivity, mode);
  hipStream_t st = cfun_st(stream);
  const unsigned per_voxel = (unsigned)(((long long)a.n + kNT - 1) / kNT);
  hipLaunchKernelGGL(k_cc_local, dim3((unsigned)tiles_of(a.D, a.H, a.W)), dim3(kNT), 0, st, pred, labels, a);
  CFUN_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_cc_seam, dim3(per_voxel), dim3(kNT), 0, st, pred, labels, a);
  CFUN_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_cc_flatten, dim3(per_voxel), dim3(kNT), 0, st, labels, a.n);
  CFUN_LAUNCH_CHECK();
  return CFUN_OK;
}

extern "C" int cfun_cc_filter(const uint8_t* pred, const int32_t* labels, const int32_t* dims, int32_t K, int32_t mode,
                              int32_t largest_only, int64_t min_voxels, uint8_t* out, int64_t* stats, void* workspace,
                              size_t workspace_bytes, cfun_stream_t stream) {
  if (!dims || !stats || (mode != CFUN_CC_CLASS && mode != CFUN_CC_FOREGROUND) || K < 1 || K > 15 || min_voxels < 0)
    return CFUN_EINVAL;
  if (!dims_ok(dims[0], dims[1], dims[2])) return CFUN_EINVAL;
  hipStream_t st = cfun_st(stream);
  if (dims[0] == 0 || dims[1] == 0 || dims[2] == 0) {
    if (hipMemsetAsync(stats, 0, (size_t)K * 3 * sizeof(int64_t), st) != hipSuccess) return CFUN_EINVAL;
    return CFUN_OK;
  }
  if (!pred || !labels || !out) return CFUN_EINVAL;
  const CcArgs a = make_args(dims[0], dims[1], dims[2], 6, mode);
  if (!workspace || workspace_bytes < cfun_cc_workspace_bytes(a.D, a.H, a.W, K)) return CFUN_EWORKSPACE;
  const int nwg = select_wg(a.n);
  int* size = (int*)workspace;
  unsigned long long* partials = (unsigned long long*)((char*)workspace + size_bytes(a.n));
  int* winner = (int*)((char*)partials + partial_bytes(a.n));
  const int fg = a.foreground;
  const unsigned per_voxel = (unsigned)(((long long)a.n + kNT - 1) / kNT);
  if (hipMemsetAsync(size, 0, (size_t)a.n * sizeof(int), st) != hipSuccess) return CFUN_EINVAL;
  hipLaunchKernelGGL(k_cc_size, dim3((unsigned)tiles_of(a.D, a.H, a.W)), dim3(kNT), 0, st, labels, size, a);
  CFUN_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_cc_select, dim3((unsigned)nwg), dim3(kNT), 0, st, pred, labels, (const int*)size, partials, a.n, (int)K, fg,
                     (long long)min_voxels, nwg);
  CFUN_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_cc_finish, dim3((unsigned)K), dim3(kNT), 0, st, (const unsigned long long*)partials, nwg, (int)largest_only,
                     (long long)min_voxels, stats, winner);
  CFUN_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_cc_write, dim3(per_voxel), dim3(kNT), 0, st, pred, labels, (const int*)size, (const int*)winner, out, a.n,
                     (int)K, fg, (int)largest_only, (long long)min_voxels);
  CFUN_LAUNCH_CHECK();
  return CFUN_OK;
}
