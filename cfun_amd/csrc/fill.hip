// Hole filling of a class map on the device (include/cfun_fill.h): scipy.ndimage.binary_fill_holes per class, or on the foreground
// as a whole, in 3-D or plane by plane, written back into the map.  Integers only; no result depends on arrival order.
//
// Per group (one in foreground mode; the classes K-1 .. 1, in that order, in class mode) five launches on the caller's stream:
//   (a) k_fill_local    a workgroup owns an 8z x 8y x 64x tile: union-find in LDS over the tile's COMPLEMENT voxels (byte != k, or
//                       byte == 0 in foreground mode) through the backward half of the neighbourhood -- 3 of 6, 13 of 26, or the
//                       2 of 4 / 4 of 8 in-plane offsets of a planar fill -- then labels[i] = 1 + the global index of the
//                       tile-local root, 0 for an object voxel.  A tile with nothing of the object in it (most tiles of a CT map)
//                       skips the union-find: it is one box, or one rectangle per plane, rooted at its first voxel
//   (b) k_fill_seam     every complement voxel on a tile boundary unites with its backward neighbours in ANOTHER tile, on labels
//                       -- but for the pairs that the pair one step back along the seam stands for (see there)
//   (c) k_fill_flatten  labels[i] = 1 + root
//   (d) k_fill_mark     the complement voxels of the counted border faces mark their root open: labels[root] = kOpen.  Every
//                       writer stores the same value with an ordinary store; only root cells are ever rewritten, and a reader
//                       that finds kOpen in its own cell knows that it is a root and already marked.  The grid covers the faces
//                       (blockIdx.y) in stretches of 256 voxels; no interior voxel is looked at.
//   (e) k_fill_write    out = the group's id where pred == 0, the voxel's root is not open and no higher group has claimed the
//                       voxel (a read of out: the higher groups' launches came before this one on the stream); the first group
//                       also copies every other byte.  Voxels changed and enclosed roots (a root cell that is not kOpen) go to
//                       per-workgroup integer partials.
// and at the end k_fill_finish, one workgroup per row of stats, adds the partials (as eval.hip and cc.hip).
//
// The forest is cc.hip's (cc_forest.h): the same cells, the same unite(), the same termination argument.  Inside a tile the local
// order (lz, ly, lx) agrees with the global order (z, y, x), so the LDS pass follows the same rule.  A planar fill is the same
// forest with fewer adjacencies: the planes never get united because no enabled offset leaves the plane.
#include "common.h"
#include "cc_forest.h"
#include "../../include/cfun_fill.h"

namespace {

constexpr int kNT = 256;
constexpr int kTZ = 8, kTY = 8, kTX = 64;             // the tile of cc.hip; kTX == the wave's width, kTZ * kTY rows
constexpr int kTile = kTZ * kTY * kTX;                // 4096 voxels: 4 KiB of complement flags, 16 KiB of parents
constexpr int kRows = kTZ * kTY, kRowsPerThread = kRows / (kNT / kTX);
constexpr int kMaxWG = 1536;                          // write pass: workgroups (as eval.hip: 6 per CU)
constexpr int kGroups = 16;                           // K <= 15
constexpr int kFields = 2;                            // per group: enclosed components, voxels changed
constexpr int kOpen = -1;                             // a root cell of an open component, after k_fill_mark

struct FillArgs {
  int D, H, W;
  int ntx, nty;              // tiles along x and y
  int n;                     // D * H * W < 2^31 - 1
  int nbr;                   // bit k: backward offset k of cc_forest.h is an adjacency of this fill
  int axis;                  // -1, or the axis the planes are perpendicular to
  int object;                // the class whose complement is labelled; -1: the foreground (complement: byte == 0)
};

__device__ __forceinline__ bool in_complement(int c, int object) { return object < 0 ? c == 0 : c != object; }

// (a) one workgroup per tile.  Thread t owns column lx = t % 64 of the rows t / 64 + 4 j: a wave reads 64 consecutive bytes.
__global__ void __launch_bounds__(kNT)
k_fill_local(const uint8_t* __restrict__ pred, int* __restrict__ labels, FillArgs a) {
  __shared__ uint8_t comp[kTile];
  __shared__ int par[kTile];
  __shared__ int mixed;                               // some voxel of the tile belongs to the object
  const int t = threadIdx.x, lx = t & (kTX - 1), r0 = t / kTX;
  const int tx = blockIdx.x % a.ntx, rest = blockIdx.x / a.ntx;
  const int ty = rest % a.nty, tz = rest / a.nty;
  const int x0 = tx * kTX, y0 = ty * kTY, z0 = tz * kTZ;
  const int x = x0 + lx;
  if (t == 0) mixed = 0;
  __syncthreads();
#pragma unroll
  for (int j = 0; j < kRowsPerThread; ++j) {
    const int row = r0 + j * (kNT / kTX), ly = row % kTY, lz = row / kTY;
    const int y = y0 + ly, z = z0 + lz;
    const int l = row * kTX + lx;
    const bool in = x < a.W && y < a.H && z < a.D;              // outside the volume: no voxel, in no component
    const bool c = in && in_complement(pred[((long long)z * a.H + y) * a.W + x], a.object);
    comp[l] = c ? 1 : 0;
    par[l] = l;
    if (in && !c) mixed = 1;                          // (every writer stores the same value)
  }
  __syncthreads();
  if (!mixed) {
    // Nine tiles in ten of a CT map: nothing of the object in it.  The tile's part of the volume is a box (of a planar fill: a
    // stack of rectangles), connected under every neighbourhood, and its smallest index is its first voxel: the forest the
    // union-find below would arrive at, written down directly.  The whole workgroup takes this branch or none of it does.
#pragma unroll 4
    for (int j = 0; j < kRowsPerThread; ++j) {
      const int row = r0 + j * (kNT / kTX), ly = row % kTY, lz = row / kTY;
      const int y = y0 + ly, z = z0 + lz;
      if (x >= a.W || y >= a.H || z >= a.D) continue;
      const int rz = a.axis == 0 ? z : z0, ry = a.axis == 1 ? y : y0, rx = a.axis == 2 ? x : x0;
      labels[((long long)z * a.H + y) * a.W + x] = (int)(((long long)rz * a.H + ry) * a.W + rx) + 1;
    }
    return;
  }
  const LdsForest f{par};
  // A planar fill that has the x step takes the runs along x first, on their own, and flattens them before anything else: a
  // wave that links its 64 voxels to their left neighbours at once builds chains as long as the runs, and with most voxels in
  // the complement the runs are whole rows; with only one other axis to merge them early, every later find() walks them.
  // Flattened, a find() starts one step from the head of its run.  Measured at 256 x 320 x 320, axis 0: 971 us without this,
  // 400 us with it.  The 3-D fill keeps the order z, y, x in one sweep: there the columns are merged, on cells of their own,
  // before x is looked at, and x-first would send the 64 lanes of a row to one cell for every z and y step (197 us against
  // 428 us).  (The flatten rewrites a cell while others walk through it: old and new value are both ancestors of the cell, as
  // in k_fill_flatten.)
  const bool x_first = a.axis >= 0 && ((a.nbr >> 12) & 1);      // offset 12 is (0, 0, -1); planes along axis 2 do not have it
  if (x_first) {
    for (int j = 0; j < kRowsPerThread; ++j) {
      const int l = (r0 + j * (kNT / kTX)) * kTX + lx;
      if (lx != 0 && comp[l] && comp[l - 1]) unite(f, l, l - 1);
    }
    __syncthreads();
    for (int j = 0; j < kRowsPerThread; ++j) {
      const int l = (r0 + j * (kNT / kTX)) * kTX + lx;
      if (comp[l]) par[l] = find(f, l);
    }
    __syncthreads();
  }
  for (int j = 0; j < kRowsPerThread; ++j) {
    const int row = r0 + j * (kNT / kTX), ly = row % kTY, lz = row / kTY;
    const int l = row * kTX + lx;
    if (!comp[l]) continue;
#pragma unroll
    for (int k = 0; k < 13; ++k) {
      if (!((a.nbr >> k) & 1) || (k == 12 && x_first)) continue;
      int dz, dy, dx;
      backward_offset(k, dz, dy, dx);
      const int nz = lz + dz, ny = ly + dy, nx = lx + dx;
      if (nz < 0 || ny < 0 || ny >= kTY || nx < 0 || nx >= kTX) continue;        // another tile: the seam pass
      const int m = (nz * kTY + ny) * kTX + nx;
      if (comp[m]) unite(f, l, m);
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
    if (comp[l]) {
      const int r = find(f, l);
      const int rx = r % kTX, ry = (r / kTX) % kTY, rz = r / (kTX * kTY);
      lab = (int)(((long long)(z0 + rz) * a.H + (y0 + ry)) * a.W + (x0 + rx)) + 1;
    }
    labels[((long long)z * a.H + y) * a.W + x] = lab;
  }
}

// (b) one thread per voxel; only a voxel on the rim of its tile can have a backward neighbour in another tile.  This is cc.hip's
// seam pass on the complement: unite() on the global array, lock-free, no workgroup waits for another, no flag, no spin; its
// termination argument (cc_forest.h: the larger of the two indices strictly decreases every round) holds unchanged, because the
// only thing that differs is WHICH pairs of voxels are handed to it.
__global__ void __launch_bounds__(kNT)
k_fill_seam(const uint8_t* __restrict__ pred, int* labels, FillArgs a) {
  const long long i64 = (long long)blockIdx.x * kNT + threadIdx.x;
  if (i64 >= a.n) return;
  const int i = (int)i64;
  const int x = i % a.W, yz = i / a.W, y = yz % a.H, z = yz / a.H;
  const int lx = x % kTX, ly = y % kTY, lz = z % kTZ;
  if (lx != 0 && lx != kTX - 1 && ly != 0 && ly != kTY - 1 && lz != 0) return;
  if (!in_complement(pred[i], a.object)) return;
  const GlobalForest f{labels};
#pragma unroll
  for (int k = 0; k < 13; ++k) {
    if (!((a.nbr >> k) & 1)) continue;
    int dz, dy, dx;
    backward_offset(k, dz, dy, dx);
    const int nz = z + dz, ny = y + dy, nx = x + dx;
    if (nz < 0 || ny < 0 || ny >= a.H || nx < 0 || nx >= a.W) continue;
    if (nz / kTZ == z / kTZ && ny / kTY == y / kTY && nx / kTX == x / kTX) continue;        // same tile: done in LDS
    const int m = (nz * a.H + ny) * a.W + nx;
    if (!in_complement(pred[m], a.object)) continue;
    // The same union as the pair one step back along the seam?  With e a unit step of this fill's neighbourhood that keeps
    // i - e in i's tile and m - e in m's tile: if both of those are complement voxels, the local pass has put i - e with i and
    // m - e with m, and the thread of i - e sees the pair (i - e, m - e) through this same offset k -- or leaves it, by this
    // same rule, to a pair further back; the chain ends because the indices decrease.  So the first pair of every run along
    // a seam does the union and the others do not queue up behind it at one cell of one cache.  Only bytes of pred are read for
    // this, which no one writes; unite() is untouched.  (lx != 0 gives x >= 1, nx % kTX != 0 gives nx >= 1; likewise y and z.)
    bool covered = false;
    if (a.axis != 2 && lx != 0 && nx % kTX != 0)
      covered = in_complement(pred[i - 1], a.object) && in_complement(pred[m - 1], a.object);
    if (!covered && a.axis != 1 && ly != 0 && ny % kTY != 0)
      covered = in_complement(pred[i - a.W], a.object) && in_complement(pred[m - a.W], a.object);
    if (!covered && a.axis != 0 && lz != 0 && nz % kTZ != 0)
      covered = in_complement(pred[i - a.H * a.W], a.object) && in_complement(pred[m - a.H * a.W], a.object);
    if (!covered) unite(f, i, m);
  }
}

// (c) in place.  A cell is rewritten with 1 + its root while other threads still walk through it: both the old and the new value
// are ancestors of the cell, so their walks end at the same root (no link is made in this launch: roots stay roots).
__global__ void __launch_bounds__(kNT)
k_fill_flatten(int* labels, int n) {
  const long long i = (long long)blockIdx.x * kNT + threadIdx.x;
  if (i >= n) return;
  const GlobalForest f{labels};
  const int p = f.parent((int)i);
  if (p < 0 || p == (int)i) return;
  labels[i] = find(f, p) + 1;
}

// (d) blockIdx.y = 2 * b + side names the face with coordinate b (0: z, 1: y, 2: x) at 0 or at its maximum; blockIdx.x walks the
// face in stretches of kNT voxels, x (or, on an x face, y) fastest.  A planar fill does not count the two faces perpendicular to
// its axis.  When an extent is 1 the two faces of that coordinate are the same voxels; they then store the same value twice.
__global__ void __launch_bounds__(kNT)
k_fill_mark(int* labels, FillArgs a) {
  const int b = blockIdx.y >> 1, side = blockIdx.y & 1;
  if (b == a.axis) return;
  const long long j = (long long)blockIdx.x * kNT + threadIdx.x;
  int z, y, x;
  if (b == 0) {
    if (j >= (long long)a.H * a.W) return;
    z = side ? a.D - 1 : 0; y = (int)(j / a.W); x = (int)(j % a.W);
  } else if (b == 1) {
    if (j >= (long long)a.D * a.W) return;
    z = (int)(j / a.W); y = side ? a.H - 1 : 0; x = (int)(j % a.W);
  } else {
    if (j >= (long long)a.D * a.H) return;
    z = (int)(j / a.H); y = (int)(j % a.H); x = side ? a.W - 1 : 0;
  }
  const int i = (int)(((long long)z * a.H + y) * a.W + x);
  const int p = labels[i];                            // 0: object; kOpen: a root, already marked; else 1 + root (flattened)
  if (p == 0) return;
  labels[p == kOpen ? i : p - 1] = kOpen;
}

// (e) a grid-stride sweep.  first: this is the first group of the call, out holds nothing yet and every byte is written; later
// groups only touch the voxels they fill.
__global__ void __launch_bounds__(kNT)
k_fill_write(const uint8_t* __restrict__ pred, const int* __restrict__ labels, uint8_t* __restrict__ out,
             unsigned long long* __restrict__ partials, int n, int value, int first, int nwg) {
  __shared__ unsigned long long acc[kFields];
  const int t = threadIdx.x;
  if (t < kFields) acc[t] = 0;
  __syncthreads();
  unsigned roots = 0, changed = 0;
  for (long long i = (long long)blockIdx.x * kNT + t; i < n; i += (long long)nwg * kNT) {
    const int c = pred[i], p = labels[i];
    bool enclosed = false;
    if (p != 0 && p != kOpen) {
      if (p == (int)i + 1) { enclosed = true; ++roots; }
      else enclosed = labels[p - 1] != kOpen;
    }
    const bool fill = enclosed && c == 0 && (first || out[i] == 0);
    if (fill) { out[i] = (uint8_t)value; ++changed; }
    else if (first) out[i] = (uint8_t)c;
  }
  if (roots) atomicAdd(&acc[0], (unsigned long long)roots);
  if (changed) atomicAdd(&acc[1], (unsigned long long)changed);
  __syncthreads();
  if (t < kFields) partials[(long long)t * nwg + blockIdx.x] = acc[t];
}

// class mode with K == 1: no group at all, the map passes through
__global__ void __launch_bounds__(kNT)
k_fill_copy(const uint8_t* __restrict__ pred, uint8_t* __restrict__ out, int n) {
  const long long i = (long long)blockIdx.x * kNT + threadIdx.x;
  if (i < n) out[i] = pred[i];
}

// one workgroup per row of stats: rows lo .. hi - 1 sum their partials, the others are zero.  Sums of integers: the order does not
// matter.
__global__ void __launch_bounds__(kNT)
k_fill_finish(const unsigned long long* __restrict__ partials, int nwg, int lo, int hi, int64_t* __restrict__ stats) {
  __shared__ unsigned long long acc[kFields];
  const int t = threadIdx.x, g = blockIdx.x;
  if (t < kFields) acc[t] = 0;
  __syncthreads();
  if (g >= lo && g < hi) {
    unsigned long long v[kFields] = {0, 0};
    for (int w = t; w < nwg; w += kNT) {
#pragma unroll
      for (int f = 0; f < kFields; ++f) v[f] += partials[(long long)(g * kFields + f) * nwg + w];
    }
#pragma unroll
    for (int f = 0; f < kFields; ++f)
      if (v[f]) atomicAdd(&acc[f], v[f]);
  }
  __syncthreads();
  if (t < kFields) stats[g * kFields + t] = (long long)acc[t];
}

bool dims_ok(int D, int H, int W) {
  if (D < 0 || H < 0 || W < 0) return false;
  if (D == 0 || H == 0 || W == 0) return true;
  const long long lim = (1ll << 31) - 1, dh = (long long)D * H;        // (dh < 2^62; dh * W only once dh is known to be small)
  return dh < lim && dh * W < lim;
}

int write_wg(long long n) {
  const long long w = (n + kNT * 16 - 1) / (kNT * 16);
  return (int)(w < kMaxWG ? w : kMaxWG);
}

// the workspace: labels[n] | partials[kGroups * kFields][nwg]
size_t label_bytes(long long n) { return cfun_align_up((size_t)n * sizeof(int), 256); }
size_t partial_bytes(long long n) { return (size_t)kGroups * kFields * write_wg(n) * sizeof(unsigned long long); }

// The adjacencies of a fill as a mask over the 13 backward offsets (the arithmetic of backward_offset(), on the host): an offset
// counts when it stays in the plane (axis >= 0: its component along axis is 0) and, with the small neighbourhood (6 or 4), has
// exactly one non-zero component.
int neighbour_mask(int axis, bool all) {
  int mask = 0;
  for (int k = 0; k < 13; ++k) {
    int d[3];
    if (k < 9) { d[0] = -1; d[1] = k / 3 - 1; d[2] = k % 3 - 1; }
    else if (k < 12) { d[0] = 0; d[1] = -1; d[2] = k - 10; }
    else { d[0] = 0; d[1] = 0; d[2] = -1; }
    if (axis >= 0 && d[axis] != 0) continue;
    const int nonzero = (d[0] != 0) + (d[1] != 0) + (d[2] != 0);
    if (all || nonzero == 1) mask |= 1 << k;
  }
  return mask;
}

}  // namespace

extern "C" size_t cfun_fill_workspace_bytes(int32_t D, int32_t H, int32_t W, int32_t K) {
  if (!dims_ok(D, H, W) || K < 1 || K > 15 || D == 0 || H == 0 || W == 0) return 0;
  const long long n = (long long)D * H * W;
  return label_bytes(n) + partial_bytes(n);
}

extern "C" int cfun_fill_holes(const uint8_t* pred, const int32_t* dims, int32_t K, int32_t mode, int32_t connectivity, int32_t axis,
                               int32_t fill_value, uint8_t* out, int64_t* stats, void* workspace, size_t workspace_bytes,
                               cfun_stream_t stream) {
  if (!dims || !stats || (mode != CFUN_CC_CLASS && mode != CFUN_CC_FOREGROUND) || K < 1 || K > 15) return CFUN_EINVAL;
  if (axis < -1 || axis > 2) return CFUN_EINVAL;
  if (axis < 0 ? (connectivity != 6 && connectivity != 26) : (connectivity != 4 && connectivity != 8)) return CFUN_EINVAL;
  if (mode == CFUN_CC_FOREGROUND && (fill_value < 1 || fill_value > 255)) return CFUN_EINVAL;
  if (!dims_ok(dims[0], dims[1], dims[2])) return CFUN_EINVAL;
  hipStream_t st = cfun_st(stream);
  if (dims[0] == 0 || dims[1] == 0 || dims[2] == 0) {
    if (hipMemsetAsync(stats, 0, (size_t)K * kFields * sizeof(int64_t), st) != hipSuccess) return CFUN_EINVAL;
    return CFUN_OK;
  }
  if (!pred || !out) return CFUN_EINVAL;
  FillArgs a;
  a.D = dims[0]; a.H = dims[1]; a.W = dims[2];
  a.ntx = (a.W + kTX - 1) / kTX;
  a.nty = (a.H + kTY - 1) / kTY;
  a.n = (int)((long long)a.D * a.H * a.W);
  a.nbr = neighbour_mask(axis, connectivity == 26 || connectivity == 8);
  a.axis = axis;
  if ((uintptr_t)out < (uintptr_t)pred + (uintptr_t)a.n && (uintptr_t)pred < (uintptr_t)out + (uintptr_t)a.n) return CFUN_EINVAL;
  if (!workspace || workspace_bytes < cfun_fill_workspace_bytes(a.D, a.H, a.W, K)) return CFUN_EWORKSPACE;
  int* labels = (int*)workspace;
  unsigned long long* partials = (unsigned long long*)((char*)workspace + label_bytes(a.n));
  const int nwg = write_wg(a.n);
  const unsigned per_voxel = (unsigned)(((long long)a.n + kNT - 1) / kNT);
  const unsigned tiles = (unsigned)((long long)((a.D + kTZ - 1) / kTZ) * a.nty * a.ntx);
  const long long dh = (long long)a.D * a.H, dw = (long long)a.D * a.W, hw = (long long)a.H * a.W;
  const long long face = dh > dw ? (dh > hw ? dh : hw) : (dw > hw ? dw : hw);
  const unsigned per_face = (unsigned)((face + kNT - 1) / kNT);
  const bool fg = mode == CFUN_CC_FOREGROUND;
  // the rows of stats that carry a group: [lo, hi)
  const int lo = fg ? 0 : 1, hi = fg ? 1 : K;
  if (lo >= hi) {
    hipLaunchKernelGGL(k_fill_copy, dim3(per_voxel), dim3(kNT), 0, st, pred, out, a.n);
    CFUN_LAUNCH_CHECK();
  }
  for (int g = hi - 1; g >= lo; --g) {
    a.object = fg ? -1 : g;
    hipLaunchKernelGGL(k_fill_local, dim3(tiles), dim3(kNT), 0, st, pred, labels, a);
    CFUN_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_fill_seam, dim3(per_voxel), dim3(kNT), 0, st, pred, labels, a);
    CFUN_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_fill_flatten, dim3(per_voxel), dim3(kNT), 0, st, labels, a.n);
    CFUN_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_fill_mark, dim3(per_face, 6), dim3(kNT), 0, st, labels, a);
    CFUN_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_fill_write, dim3((unsigned)nwg), dim3(kNT), 0, st, pred, (const int*)labels, out,
                       partials + (size_t)g * kFields * nwg, a.n, fg ? (int)fill_value : g, g == hi - 1 ? 1 : 0, nwg);
    CFUN_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(k_fill_finish, dim3((unsigned)K), dim3(kNT), 0, st, (const unsigned long long*)partials, nwg, lo, hi, stats);
  CFUN_LAUNCH_CHECK();
  return CFUN_OK;
}
