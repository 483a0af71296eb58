// Surface distances between two class maps on the device (include/cfun_surface.h): the surface voxels of a class, the exact
// squared Euclidean distance field of that surface, and per class the sums, maxima and order statistics behind Hausdorff, HD95,
// ASSD and RMSD.  Built with -ffp-contract=off: the field is defined float32 operation by float32 operation.
//
// cfun_surface_field
//   (a) k_surface     one thread per voxel: 1 where the map holds the class and a face neighbour does not (or is outside)
//   (b) k_sweep_x     x: a workgroup stages a slab of whole rows (consecutive in memory) in LDS as 0 / +inf; one thread per row
//                     walks it both ways for the index distance k to the row's nearest surface voxel; out = fl(float(k * k) * sx2)
//   (c) k_sweep<1>    y: a slab of whole y lines of one z plane, kMaxLines or fewer columns wide, x-contiguous in LDS and in
//   (d) k_sweep<2>    z: memory; the same for whole z lines of one y.  In place: a workgroup reads and writes its own lines only
//       Every thread owns one output voxel at a time and scans outwards from it in both directions, inside the line's range of
//       finite cells only; it stops once fl(float(k * k) * a2) >= best (every later candidate is at least that) and skips a line
//       whose staged values are all +inf.  The minimum over the candidates it does look at is the minimum over all.
// cfun_surface_stats, per class, both maps in one launch of (a) .. (d) (blockIdx.y), then
//   (e) k_gather      at A's voxels B's field and the reverse: count, sum d, sum d^2, max and the first radix histogram, fp64
//       k_finish      partials per workgroup; one workgroup adds them in a fixed order and sets up the selection
//   (f) k_hist        radix selection over the uint32 patterns of d^2 (monotone for non-negative floats), 11 + 11 + 10 bits:
//       k_pick        LDS histograms of the keys under the current prefix, flushed with integer atomicAdd; one workgroup
//                     finds the bin that holds each of the two ranks and writes the next prefix and residual rank to memory
//
// Workgroups talk only through integer atomics on global memory and through kernel boundaries; no thread waits for a value
// another workgroup writes, and every loop is bounded by a line length or a grid stride.
#include "common.h"
#include "../../include/cfun_surface.h"

namespace {

constexpr int kNT = 256;
constexpr int kMaxDim = 4096;                         // float(k * k) is exact below 2^24
constexpr int kSlabFloats = 10240;                    // a sweep's slab: 40 KiB of LDS, 3 or 4 workgroups per CU
constexpr int kMaxLines = 64;                         // lines per slab at most: one wave across x
constexpr int kGatherWG = 1024;                       // (e), (f): workgroups at most, 4 per CU
constexpr int kVoxPerThread = 16;
constexpr int kBins = 2048;                           // 11 bits
constexpr int kPasses = 3;                            // 11 + 11 + 10

static_assert(kSlabFloats >= kMaxDim + 1, "a slab holds at least one whole line");
static_assert(kNT % kMaxLines == 0, "whole groups of threads per line");

__device__ __forceinline__ float inf32() { return __builtin_huge_valf(); }
__device__ __forceinline__ unsigned bits_of(float v) { return __builtin_bit_cast(unsigned, v); }
__device__ __forceinline__ float float_of(unsigned v) { return __builtin_bit_cast(float, v); }

// (a) blockIdx.y picks the map
__global__ void __launch_bounds__(kNT)
k_surface(const uint8_t* __restrict__ m0, const uint8_t* __restrict__ m1, uint8_t* __restrict__ s0, uint8_t* __restrict__ s1,
          int D, int H, int W, int n, int cls) {
  const long long i64 = (long long)blockIdx.x * kNT + threadIdx.x;
  if (i64 >= n) return;
  const int i = (int)i64;
  const uint8_t* __restrict__ m = blockIdx.y ? m1 : m0;
  uint8_t* __restrict__ s = blockIdx.y ? s1 : s0;
  const int x = i % W, yz = i / W, y = yz % H, z = yz / H, hw = H * W;
  bool on = false;
  if (m[i] == cls)
    on = x == 0 || m[i - 1] != cls || x == W - 1 || m[i + 1] != cls || y == 0 || m[i - W] != cls || y == H - 1 ||
         m[i + W] != cls || z == 0 || m[i - hw] != cls || z == D - 1 || m[i + hw] != cls;
  s[i] = on ? (uint8_t)1 : (uint8_t)0;
}

struct SweepArgs {
  int D, H, W;
  int L;                     // the line's length: W, H or D
  int lines;                 // lines per slab: rows (x sweep) or columns (y and z sweeps)
  int tiles_x;               // y and z sweeps: slabs along x
  float a2;
};

// (b) The slab is `lines` whole rows, consecutive in memory, staged as 0 / +inf with a row stride of W + 1 floats (so that the
// threads of the serial pass below, one per row, fall into different banks).  One thread per row then walks its row forwards and
// backwards and leaves in every cell the index distance k to the nearest surface voxel of the row (+inf when there is none): a
// float count, exact up to 4096.  fl(float(k * k) * a2) is monotone in k, so its minimum over the row's surface voxels is its
// value at that smallest k -- the same bits as the scan over all of them.
__global__ void __launch_bounds__(kNT)
k_sweep_x(const uint8_t* __restrict__ surf0, const uint8_t* __restrict__ surf1, float* __restrict__ field0, float* __restrict__ field1,
          SweepArgs a) {
  __shared__ float g[kSlabFloats];
  const int t = threadIdx.x, W = a.W, S = a.W + 1;
  const uint8_t* __restrict__ surf = blockIdx.y ? surf1 : surf0;
  float* __restrict__ field = blockIdx.y ? field1 : field0;
  const long long rows = (long long)a.D * a.H, r0 = (long long)blockIdx.x * a.lines;
  const int nl = rows - r0 < a.lines ? (int)(rows - r0) : a.lines;
  const long long base = r0 * W;
  const int cnt = nl * W;                                                    // nl * (W + 1) <= kSlabFloats
  for (int o = t; o < cnt; o += kNT) {
    const int c = o / W, p = o - c * W;
    g[c * S + p] = surf[base + o] ? 0.f : inf32();
  }
  __syncthreads();
  if (t < nl) {
    float* row = g + t * S;
    float d = inf32();
    for (int q = 0; q < W; ++q) {
      d = row[q] == 0.f ? 0.f : d + 1.f;                                     // (inf + 1 = inf)
      row[q] = d;
    }
    d = inf32();
    for (int q = W - 1; q >= 0; --q) {
      const float v = row[q];
      d = v == 0.f ? 0.f : d + 1.f;
      row[q] = v < d ? v : d;
    }
  }
  __syncthreads();
  for (int o = t; o < cnt; o += kNT) {
    const int c = o / W, p = o - c * W;
    const float k = g[c * S + p];
    field[base + o] = (k * k) * a.a2;                                        // k * k: an integer below 2^24, or +inf
  }
}

// (c) (d).  The slab is [L][lines], column fastest: consecutive threads hold consecutive addresses, in LDS and in memory.  Four
// threads per line first find the line's first and last finite cell; every candidate outside that range is +inf and is never
// looked at.  The scan takes two steps of k per round with the four cells loaded up front (at clamped, always valid addresses),
// and tests and updates them in the order of k.
template <int AXIS>
__global__ void __launch_bounds__(kNT)
k_sweep(float* field0, float* field1, SweepArgs a) {
  __shared__ float g[kSlabFloats];
  __shared__ int part_lo[kNT / kMaxLines][kMaxLines], part_hi[kNT / kMaxLines][kMaxLines];
  __shared__ int line_lo[kMaxLines], line_hi[kMaxLines];
  constexpr int kParts = kNT / kMaxLines;
  const int t = threadIdx.x, L = a.L;
  float* field = blockIdx.y ? field1 : field0;
  const int tx = blockIdx.x % a.tiles_x, outer = blockIdx.x / a.tiles_x;      // outer: the z plane (y sweep) or the y row (z sweep)
  const int x0 = tx * a.lines;
  const int nl = a.W - x0 < a.lines ? a.W - x0 : a.lines;
  const long long base = AXIS == 1 ? (long long)outer * a.H * a.W + x0 : (long long)outer * a.W + x0;
  const long long pstride = AXIS == 1 ? (long long)a.W : (long long)a.H * a.W;
  const int cnt = nl * L;                                                    // <= kSlabFloats
  for (int o = t; o < cnt; o += kNT) {
    const int p = o / nl, c = o - p * nl;
    g[o] = field[base + p * pstride + c];
  }
  __syncthreads();
  {
    const int c = t % kMaxLines, part = t / kMaxLines;
    const int len = (L + kParts - 1) / kParts, q0 = part * len, q1 = q0 + len < L ? q0 + len : L;
    int lo = L, hi = -1;
    if (c < nl)
      for (int q = q0; q < q1; ++q)
        if (g[q * nl + c] < inf32()) {
          lo = q < lo ? q : lo;
          hi = q;
        }
    part_lo[part][c] = lo;
    part_hi[part][c] = hi;
  }
  __syncthreads();
  if (t < kMaxLines) {
    int lo = L, hi = -1;
#pragma unroll
    for (int part = 0; part < kParts; ++part) {
      lo = part_lo[part][t] < lo ? part_lo[part][t] : lo;
      hi = part_hi[part][t] > hi ? part_hi[part][t] : hi;
    }
    line_lo[t] = lo;
    line_hi[t] = hi;
  }
  __syncthreads();
  for (int o = t; o < cnt; o += kNT) {
    const int p = o / nl, c = o - p * nl;
    const int lo = line_lo[c], hi = line_hi[c];
    float best = g[o];
    if (hi >= 0) {                                                           // else every cell of the line is +inf
      const int kmax = p - lo > hi - p ? p - lo : hi - p;
      int k = p < lo ? lo - p : p > hi ? p - hi : 1;
      k = k < 1 ? 1 : k;
      for (; k <= kmax; k += 2) {
        const int jl0 = p - k, jr0 = p + k, jl1 = jl0 - 1, jr1 = jr0 + 1;
        const float l0 = g[(jl0 < lo ? lo : jl0) * nl + c], r0 = g[(jr0 > hi ? hi : jr0) * nl + c];
        const float l1 = g[(jl1 < lo ? lo : jl1) * nl + c], r1 = g[(jr1 > hi ? hi : jr1) * nl + c];
        const float t0 = (float)(k * k) * a.a2;
        if (t0 >= best) break;
        float cand = jl0 >= lo ? l0 + t0 : inf32();
        best = cand < best ? cand : best;
        cand = jr0 <= hi ? r0 + t0 : inf32();
        best = cand < best ? cand : best;
        const float t1 = (float)((k + 1) * (k + 1)) * a.a2;
        if (t1 >= best) break;
        cand = jl1 >= lo ? l1 + t1 : inf32();
        best = cand < best ? cand : best;
        cand = jr1 <= hi ? r1 + t1 : inf32();
        best = cand < best ? cand : best;
      }
    }
    field[base + p * pstride + c] = best;
  }
}

// ---- (e)
struct Partial {
  long long cnt;
  double sum, sumsq;
  float mx;
  int pad;
};

struct SelState {
  unsigned long long rank[2];
  unsigned prefix[2];
  int empty, pad;
};

struct Acc {
  long long cnt = 0;
  double sum = 0.0, sumsq = 0.0;
  float mx = 0.f;
  __device__ __forceinline__ void add(float d2) {
    const double v = (double)d2;
    ++cnt;
    sum += sqrt(v);
    sumsq += v;
    mx = d2 > mx ? d2 : mx;
  }
  __device__ __forceinline__ void merge(long long c, double s, double q, float m) {
    cnt += c; sum += s; sumsq += q; mx = m > mx ? m : mx;
  }
  __device__ __forceinline__ void wave_reduce() {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1)
      merge(__shfl_xor(cnt, o, 64), __shfl_xor(sum, o, 64), __shfl_xor(sumsq, o, 64), __shfl_xor(mx, o, 64));
  }
};

// Reduce the two accumulators of every thread of the workgroup; thread 0 returns with the totals (waves added in order).
__device__ __forceinline__ void block_reduce(Acc& a0, Acc& a1) {
  __shared__ long long r_cnt[2][kNT / 64];
  __shared__ double r_sum[2][kNT / 64], r_sumsq[2][kNT / 64];
  __shared__ float r_mx[2][kNT / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  a0.wave_reduce();
  a1.wave_reduce();
  if (lane == 0) {
    r_cnt[0][wave] = a0.cnt; r_sum[0][wave] = a0.sum; r_sumsq[0][wave] = a0.sumsq; r_mx[0][wave] = a0.mx;
    r_cnt[1][wave] = a1.cnt; r_sum[1][wave] = a1.sum; r_sumsq[1][wave] = a1.sumsq; r_mx[1][wave] = a1.mx;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    a0 = Acc();
    a1 = Acc();
    for (int w = 0; w < kNT / 64; ++w) {
      a0.merge(r_cnt[0][w], r_sum[0][w], r_sumsq[0][w], r_mx[0][w]);
      a1.merge(r_cnt[1][w], r_sum[1][w], r_sumsq[1][w], r_mx[1][w]);
    }
  }
}

// a grid-stride sweep; also the first radix pass (every key is under the empty prefix): hist[0 .. kBins)
__global__ void __launch_bounds__(kNT)
k_gather(const uint8_t* __restrict__ surfA, const uint8_t* __restrict__ surfB, const float* __restrict__ fieldA,
         const float* __restrict__ fieldB, int n, int nwg, Partial* __restrict__ partials, unsigned* __restrict__ hist) {
  __shared__ unsigned h[kBins];
  const int t = threadIdx.x;
  for (int s = t; s < kBins; s += kNT) h[s] = 0;
  __syncthreads();
  Acc pl, lp;
  for (long long i = (long long)blockIdx.x * kNT + t; i < n; i += (long long)nwg * kNT) {
    if (surfA[i]) {
      const float d2 = fieldB[i];
      pl.add(d2);
      atomicAdd(&h[bits_of(d2) >> 21], 1u);
    }
    if (surfB[i]) {
      const float d2 = fieldA[i];
      lp.add(d2);
      atomicAdd(&h[bits_of(d2) >> 21], 1u);
    }
  }
  __syncthreads();
  for (int s = t; s < kBins; s += kNT)
    if (h[s] != 0) atomicAdd(&hist[s], h[s]);
  block_reduce(pl, lp);
  if (t == 0) {
    partials[blockIdx.x] = Partial{pl.cnt, pl.sum, pl.sumsq, pl.mx, 0};
    partials[nwg + blockIdx.x] = Partial{lp.cnt, lp.sum, lp.sumsq, lp.mx, 0};
  }
}

// one workgroup: thread t adds the partials t, t + 256, .. in that order, then the waves in order
__global__ void __launch_bounds__(kNT)
k_finish(const Partial* __restrict__ partials, int nwg, double qf, CfunSurfaceStats* __restrict__ row, SelState* __restrict__ st) {
  Acc pl, lp;
  for (int w = threadIdx.x; w < nwg; w += kNT) {
    const Partial a = partials[w], b = partials[nwg + w];
    pl.merge(a.cnt, a.sum, a.sumsq, a.mx);
    lp.merge(b.cnt, b.sum, b.sumsq, b.mx);
  }
  block_reduce(pl, lp);
  if (threadIdx.x != 0) return;
  const bool empty = pl.cnt == 0 || lp.cnt == 0;
  CfunSurfaceStats r;
  r.n_pred = pl.cnt;
  r.n_label = lp.cnt;
  r.sum_pl = empty ? 0.0 : pl.sum;
  r.sum_lp = empty ? 0.0 : lp.sum;
  r.sumsq_pl = empty ? 0.0 : pl.sumsq;
  r.sumsq_lp = empty ? 0.0 : lp.sumsq;
  r.max_sq_pl = empty ? 0.0 : (double)pl.mx;
  r.max_sq_lp = empty ? 0.0 : (double)lp.mx;
  r.q_lo_sq = 0.0;
  r.q_hi_sq = 0.0;
  r.frac = 0.0;
  SelState s;
  s.rank[0] = s.rank[1] = 0;
  s.prefix[0] = s.prefix[1] = 0;
  s.empty = empty ? 1 : 0;
  s.pad = 0;
  if (!empty) {
    const long long total = pl.cnt + lp.cnt;
    const double pos = (double)(total - 1) * qf;
    long long lo = (long long)floor(pos);
    lo = lo > total - 1 ? total - 1 : lo;
    const long long hi = lo + 1 < total - 1 ? lo + 1 : total - 1;
    r.frac = pos - (double)lo;
    s.rank[0] = (unsigned long long)lo;
    s.rank[1] = (unsigned long long)hi;
  }
  *row = r;
  *st = s;
}

// ---- (f)
__device__ __forceinline__ int prefix_shift(int pass) { return pass == 1 ? 21 : 10; }      // the bits passes before `pass` fixed
__device__ __forceinline__ int digit_shift(int pass) { return pass == 0 ? 21 : pass == 1 ? 10 : 0; }
__device__ __forceinline__ unsigned digit_mask(int pass) { return pass == 2 ? 1023u : 2047u; }

// passes 1 and 2: row r of hist counts the keys whose higher bits equal rank r's prefix
__global__ void __launch_bounds__(kNT)
k_hist(const uint8_t* __restrict__ surfA, const uint8_t* __restrict__ surfB, const float* __restrict__ fieldA,
       const float* __restrict__ fieldB, int n, int nwg, const SelState* __restrict__ st, int pass, unsigned* __restrict__ hist) {
  __shared__ unsigned h[2 * kBins];
  const int t = threadIdx.x;
  if (st->empty) return;                              // (the same answer in every thread of the grid)
  const unsigned p0 = st->prefix[0], p1 = st->prefix[1], mask = digit_mask(pass);
  const int ps = prefix_shift(pass), ds = digit_shift(pass);
  for (int s = t; s < 2 * kBins; s += kNT) h[s] = 0;
  __syncthreads();
  for (long long i = (long long)blockIdx.x * kNT + t; i < n; i += (long long)nwg * kNT) {
    if (surfA[i]) {
      const unsigned key = bits_of(fieldB[i]);
      if (key >> ps == p0) atomicAdd(&h[(key >> ds) & mask], 1u);
      if (key >> ps == p1) atomicAdd(&h[kBins + ((key >> ds) & mask)], 1u);
    }
    if (surfB[i]) {
      const unsigned key = bits_of(fieldA[i]);
      if (key >> ps == p0) atomicAdd(&h[(key >> ds) & mask], 1u);
      if (key >> ps == p1) atomicAdd(&h[kBins + ((key >> ds) & mask)], 1u);
    }
  }
  __syncthreads();
  for (int s = t; s < 2 * kBins; s += kNT)
    if (h[s] != 0) atomicAdd(&hist[s], h[s]);
}

// One workgroup.  For each of the two ranks: thread t owns the bins 8 t .. 8 t + 7, an inclusive scan over the 256 sums says
// which thread's bins hold the rank, and that thread walks its eight.  Clears the histograms for the next pass; the last pass
// writes the two order statistics into the class's row.
__global__ void __launch_bounds__(kNT)
k_pick(unsigned* __restrict__ hist, SelState* __restrict__ st, int pass, CfunSurfaceStats* __restrict__ row) {
  __shared__ unsigned long long scan[kNT];
  __shared__ unsigned long long new_rank[2];
  __shared__ unsigned new_prefix[2];
  constexpr int kPer = kBins / kNT;
  const int t = threadIdx.x;
  const int empty = st->empty;
  const unsigned long long rank0 = st->rank[0], rank1 = st->rank[1];
  const unsigned prefix0 = st->prefix[0], prefix1 = st->prefix[1];
  if (t < 2) {
    new_rank[t] = t ? rank1 : rank0;
    new_prefix[t] = t ? prefix1 : prefix0;
  }
  for (int r = 0; r < 2; ++r) {
    const unsigned* h = hist + (pass == 0 ? 0 : r * kBins);
    const unsigned long long rank = r ? rank1 : rank0;
    const unsigned prefix = r ? prefix1 : prefix0;
    unsigned long long mine = 0;
#pragma unroll
    for (int j = 0; j < kPer; ++j) mine += h[t * kPer + j];
    scan[t] = mine;
    __syncthreads();
    for (int off = 1; off < kNT; off <<= 1) {
      const unsigned long long v = t >= off ? scan[t - off] : 0;
      __syncthreads();
      scan[t] += v;
      __syncthreads();
    }
    unsigned long long before = scan[t] - mine;
    if (!empty && rank >= before && rank < before + mine) {
      for (int j = 0; j < kPer; ++j) {
        const unsigned c = h[t * kPer + j];
        if (rank < before + c) {
          new_rank[r] = rank - before;
          new_prefix[r] = pass == 0 ? (unsigned)(t * kPer + j)
                                    : (prefix << (pass == 1 ? 11 : 10)) | (unsigned)(t * kPer + j);
          break;
        }
        before += c;
      }
    }
    __syncthreads();
  }
  for (int s = t; s < 2 * kBins; s += kNT) hist[s] = 0;
  if (t == 0) {
    st->rank[0] = new_rank[0];
    st->rank[1] = new_rank[1];
    st->prefix[0] = new_prefix[0];
    st->prefix[1] = new_prefix[1];
    if (pass == kPasses - 1 && !empty) {
      row->q_lo_sq = (double)float_of(new_prefix[0]);
      row->q_hi_sq = (double)float_of(new_prefix[1]);
    }
  }
}

// ---- host
bool dims_ok(const int32_t* d) {
  if (!d) return false;
  for (int i = 0; i < 3; ++i)
    if (d[i] < 0 || d[i] > kMaxDim) return false;
  return (long long)d[0] * d[1] * d[2] < (1ll << 31) - 1;                    // (<= 2^36: no overflow)
}

bool spacing_ok(const float* s2) {
  if (!s2) return false;
  for (int i = 0; i < 3; ++i)
    if (!(s2[i] > 0.f) || !(s2[i] < __builtin_huge_valf())) return false;  // (NaN fails the first test)
  return true;
}

int gather_wg(long long n) {
  const long long w = (n + kNT * kVoxPerThread - 1) / (kNT * kVoxPerThread);
  return (int)(w < kGatherWG ? w : kGatherWG);
}

int pow2_floor(int v) {
  int p = 1;
  while (p * 2 <= v) p *= 2;
  return p;
}

// lines per slab: as many whole lines as fit, kMaxLines at most; a power of two of columns for the y and z sweeps
int slab_lines(int axis, int L) {
  const int per = axis == 0 ? L + 1 : L;                                      // (the x sweep pads a row by one float)
  const int fit = kSlabFloats / per < kMaxLines ? kSlabFloats / per : kMaxLines;
  return axis == 0 ? fit : pow2_floor(fit);
}

// the workspace of cfun_surface_stats: surfA[n] | surfB[n] | fieldA[n] | fieldB[n] | partials[2][nwg] | hist[2][kBins] | state
struct Layout {
  size_t surf, field, partials, hist, total;
};
Layout layout_of(long long n) {
  Layout l;
  l.surf = cfun_align_up((size_t)n, 256);
  l.field = cfun_align_up((size_t)n * sizeof(float), 256);
  l.partials = cfun_align_up((size_t)2 * gather_wg(n) * sizeof(Partial), 256);
  l.hist = (size_t)2 * kBins * sizeof(unsigned);
  l.total = 2 * l.surf + 2 * l.field + l.partials + l.hist + cfun_align_up(sizeof(SelState), 256);
  return l;
}

// (a) .. (d) for one map (s1 == nullptr) or two
int enqueue_field(const uint8_t* m0, const uint8_t* m1, uint8_t* s0, uint8_t* s1, float* f0, float* f1, int D, int H, int W, int cls,
                  const float* spacing2, hipStream_t st) {
  const int n = (int)((long long)D * H * W);
  const unsigned maps = s1 ? 2 : 1;
  hipLaunchKernelGGL(k_surface, dim3((unsigned)(((long long)n + kNT - 1) / kNT), maps), dim3(kNT), 0, st, m0, m1, s0, s1, D, H, W, n,
                     cls);
  CFUN_LAUNCH_CHECK();
  SweepArgs a;
  a.D = D; a.H = H; a.W = W;
  a.L = W; a.lines = slab_lines(0, W); a.tiles_x = 1; a.a2 = spacing2[2];
  const long long rows = (long long)D * H;
  hipLaunchKernelGGL(k_sweep_x, dim3((unsigned)((rows + a.lines - 1) / a.lines), maps), dim3(kNT), 0, st, (const uint8_t*)s0,
                     (const uint8_t*)s1, f0, f1, a);
  CFUN_LAUNCH_CHECK();
  a.L = H; a.lines = slab_lines(1, H); a.tiles_x = (W + a.lines - 1) / a.lines; a.a2 = spacing2[1];
  hipLaunchKernelGGL(k_sweep<1>, dim3((unsigned)((long long)D * a.tiles_x), maps), dim3(kNT), 0, st, f0, f1, a);
  CFUN_LAUNCH_CHECK();
  a.L = D; a.lines = slab_lines(2, D); a.tiles_x = (W + a.lines - 1) / a.lines; a.a2 = spacing2[0];
  hipLaunchKernelGGL(k_sweep<2>, dim3((unsigned)((long long)H * a.tiles_x), maps), dim3(kNT), 0, st, f0, f1, a);
  CFUN_LAUNCH_CHECK();
  return CFUN_OK;
}

}  // namespace

extern "C" size_t cfun_surface_workspace_bytes(int32_t D, int32_t H, int32_t W, int32_t K) {
  const int32_t d[3] = {D, H, W};
  if (!dims_ok(d) || K < 1 || K > 15 || D == 0 || H == 0 || W == 0) return 0;
  return layout_of((long long)D * H * W).total;
}

extern "C" int cfun_surface_field(const uint8_t* map, const int32_t* dims, int32_t cls, const float* spacing2, uint8_t* surface_out,
                                  float* field_out, void* workspace, size_t workspace_bytes, cfun_stream_t stream) {
  (void)workspace; (void)workspace_bytes;
  if (!dims_ok(dims) || cls < 1 || cls > 255 || !spacing_ok(spacing2)) return CFUN_EINVAL;
  if (dims[0] == 0 || dims[1] == 0 || dims[2] == 0) return CFUN_OK;
  if (!map || !surface_out || !field_out) return CFUN_EINVAL;
  return enqueue_field(map, nullptr, surface_out, nullptr, field_out, nullptr, dims[0], dims[1], dims[2], cls, spacing2,
                       cfun_st(stream));
}

extern "C" int cfun_surface_stats(const uint8_t* pred, const uint8_t* label, const int32_t* dims, int32_t K, const float* spacing2,
                                  double qf, CfunSurfaceStats* stats, void* workspace, size_t workspace_bytes,
                                  cfun_stream_t stream) {
  if (!dims_ok(dims) || K < 1 || K > 15 || !spacing_ok(spacing2) || !(qf >= 0.0 && qf <= 1.0) || !stats) return CFUN_EINVAL;
  hipStream_t st = cfun_st(stream);
  const int D = dims[0], H = dims[1], W = dims[2];
  if (D == 0 || H == 0 || W == 0) {
    if (hipMemsetAsync(stats, 0, (size_t)K * sizeof(CfunSurfaceStats), st) != hipSuccess) return CFUN_EINVAL;
    return CFUN_OK;
  }
  if (!pred || !label) return CFUN_EINVAL;
  const long long n64 = (long long)D * H * W;
  const Layout l = layout_of(n64);
  if (!workspace || workspace_bytes < l.total) return CFUN_EWORKSPACE;
  const int n = (int)n64, nwg = gather_wg(n64);
  char* w = (char*)workspace;
  uint8_t* surfA = (uint8_t*)w;
  uint8_t* surfB = (uint8_t*)(w + l.surf);
  float* fieldA = (float*)(w + 2 * l.surf);
  float* fieldB = (float*)(w + 2 * l.surf + l.field);
  Partial* partials = (Partial*)(w + 2 * l.surf + 2 * l.field);
  unsigned* hist = (unsigned*)((char*)partials + l.partials);
  SelState* state = (SelState*)((char*)hist + l.hist);
  if (hipMemsetAsync(stats, 0, (size_t)K * sizeof(CfunSurfaceStats), st) != hipSuccess) return CFUN_EINVAL;
  if (hipMemsetAsync(hist, 0, l.hist, st) != hipSuccess) return CFUN_EINVAL;      // (k_pick leaves it cleared after every pass)
  for (int c = 1; c < K; ++c) {
    const int rc = enqueue_field(pred, label, surfA, surfB, fieldA, fieldB, D, H, W, c, spacing2, st);
    if (rc != CFUN_OK) return rc;
    hipLaunchKernelGGL(k_gather, dim3((unsigned)nwg), dim3(kNT), 0, st, (const uint8_t*)surfA, (const uint8_t*)surfB,
                       (const float*)fieldA, (const float*)fieldB, n, nwg, partials, hist);
    CFUN_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_finish, dim3(1), dim3(kNT), 0, st, (const Partial*)partials, nwg, qf, stats + c, state);
    CFUN_LAUNCH_CHECK();
    for (int pass = 0; pass < kPasses; ++pass) {
      if (pass > 0) {
        hipLaunchKernelGGL(k_hist, dim3((unsigned)nwg), dim3(kNT), 0, st, (const uint8_t*)surfA, (const uint8_t*)surfB,
                           (const float*)fieldA, (const float*)fieldB, n, nwg, (const SelState*)state, pass, hist);
        CFUN_LAUNCH_CHECK();
      }
      hipLaunchKernelGGL(k_pick, dim3(1), dim3(kNT), 0, st, hist, state, pass, stats + c);
      CFUN_LAUNCH_CHECK();
    }
  }
  return CFUN_OK;
}
