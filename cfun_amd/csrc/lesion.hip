// Lesion-level scoring on the device (include/cfun_lesion.h): dense ranks and a component table from the labels of cc.hip, and the
// contingency table of two rank volumes.  Integers only; no float, no result that depends on arrival order.
//
// cfun_cc_rank      a root is a voxel whose label is 1 + its own index; a component's rank is 1 + the number of roots before its own
//   (a) k_rank_count   roots per chunk of kChunk consecutive voxels (one workgroup per chunk, 64 consecutive dwords per wave load)
//   (b) k_rank_scan    ONE workgroup turns the chunk counts into exclusive offsets, kScanNT chunks per round; writes count and the
//                      two table rows that belong to no single component (background, overflow)
//   (c) k_rank_roots   per chunk again: a local scan of the roots (a ballot per 64 voxels, one barrier for the four waves'
//                      totals), the rank written at each root, the root's table row opened
//   (d) k_rank_assign  a workgroup takes 4z x 8y x 64x tiles, one at a time: every voxel gets the rank stored at its root; sizes and boxes are
//                      aggregated per label in an LDS table (as k_cc_size: runs of equal labels, the box as occupancy bit masks
//                      of the tile's z, y and x) and reach the table as one integer update per (tile, component) and field;
//                      the components beyond cap share one row, so the tile gathers its share of that row in LDS first
// cfun_rank_overlap
//   (e) k_rank_overlap a workgroup sweeps a contiguous span of the two volumes, a wave 64 consecutive voxels per load, kU loads of
//                      each volume in flight, unconditional (a lane past the end re-reads the last voxel and counts nothing).
//                      The pair (0, 0) is counted in a register and reduced once per wave.  Of the other pairs only the first
//                      lane of a run of equal pairs touches LDS: it adds the run's length, read off a ballot, to an open-
//                      addressing table keyed by the cell index.  At the end: one global 64-bit add per used slot.  A pair that
//                      finds neither its key nor a free slot within kMaxProbe slots of its hash -- the table is full there --
//                      goes to global memory at once instead, so the probe is bounded and waits for nobody.
//
// Workgroups talk only through integer atomics on global memory and through kernel boundaries: no look-back scan, no flag, no
// ticket, no spin on a value someone else must write; every loop below has a bound that is known when it starts.
//
// What the compiler reports (gfx950, -O3, -Rpass-analysis=kernel-resource-usage); no kernel uses scratch:
//   kernel            VGPRs   SGPRs   LDS bytes   waves per SIMD   waves per CU
//   k_rank_count       22      16          16   8                32
//   k_rank_scan          17      40       1 024   8                32 (one workgroup is launched)
//   k_rank_roots       64      72          16   8                32
//   k_rank_assign        40      57      41 008   3                12 (LDS: three workgroups per CU)
//   k_rank_overlap       28      61      16 400   8                32
#include "common.h"
#include "../../include/cfun_lesion.h"

namespace {

constexpr int kNT = 256, kWaves = kNT / 64;
constexpr int kChunk = 4096;                          // voxels per chunk of the root scan
constexpr int kPerThread = kChunk / kNT;              // voxels a thread of (a) and (c) owns
constexpr int kScanNT = 256;                          // threads of the one scan workgroup = chunks per round
constexpr int kTZ = 4, kTY = 8, kTX = 64;             // the tile of (d); kTX == the wave's width
constexpr int kTile = kTZ * kTY * kTX;                // 2048 voxels, at most 2048 distinct labels: 5 x 8 KiB of LDS
constexpr int kRows = kTZ * kTY, kRowsPerThread = kRows / kWaves;
constexpr int kAssignWG = 768;                        // workgroups of (d): three per CU, as many as its LDS admits
constexpr int kF = CFUN_LESION_FIELDS;
constexpr int kU = 4;                                 // (e): loads of each volume a wave has in flight
constexpr int kStep = kNT * kU;                       // voxels a workgroup takes per step
constexpr int kMinSteps = 16;                         // steps a workgroup takes before the grid grows
constexpr int kMaxWG = 2048;                          // 8 per CU of the MI355X's 256
constexpr int kPairSlots = 2048;                      // the LDS table of (e): 16 KiB
constexpr int kMaxProbe = 32;                         // slots looked at from the hash before the pair goes to global memory

static_assert(kScanNT == kNT && kTX == 64 && kTile <= 4096, "");
constexpr int kHashShift = 21;                        // a 32-bit product's top 11 bits: a slot of either table
static_assert(kPairSlots == 1 << (32 - kHashShift) && kTile == kPairSlots && kMaxProbe <= kPairSlots, "");

// ---- what tests/emu/hip/hip_runtime.h does not have.  Its fibers switch at rendezvous points only and its workgroups run one
// after another, so a plain read-modify-write is atomic there (as cc.hip).
#ifdef CFUN_HIP_EMULATION
__device__ __forceinline__ int rk_cas(int* p, int expect, int v) { const int o = *p; if (o == expect) *p = v; return o; }
__device__ __forceinline__ void rk_or(unsigned* p, unsigned v) { *p |= v; }
__device__ __forceinline__ int rk_load_lds(const int* p) { return *p; }
__device__ __forceinline__ long long rk_load_global64(const int64_t* p) { return *p; }
__device__ __forceinline__ void rk_min32(int* p, int v) { if (v < *p) *p = v; }
__device__ __forceinline__ void rk_max32(int* p, int v) { if (v > *p) *p = v; }
__device__ __forceinline__ void rk_min64(int64_t* p, long long v) { if (v < *p) *p = v; }
__device__ __forceinline__ void rk_max64(int64_t* p, long long v) { if (v > *p) *p = v; }
// one rendezvous of the wave: bit l of the result is lane l's predicate; *prev is the value of the lane before (of lane 0: its own)
__device__ __forceinline__ unsigned long long rk_ballot_prev(int pred, int v, int* prev) {
  const int mine[2] = {pred, v};
  const hipemu::Slot* s = hipemu::wave_exchange(mine, sizeof(mine));
  unsigned long long m = 0;
  for (int l = 0; l < 64; ++l) {
    int p;
    memcpy(&p, s[l].b, 4);
    if (p) m |= 1ull << l;
  }
  const int lane = hipemu::lane_id();
  memcpy(prev, s[lane ? lane - 1 : 0].b + 4, 4);
  return m;
}
__device__ __forceinline__ unsigned long long rk_ballot(int pred) {
  int unused;
  return rk_ballot_prev(pred, 0, &unused);
}
#else
__device__ __forceinline__ int rk_cas(int* p, int expect, int v) { return atomicCAS(p, expect, v); }
__device__ __forceinline__ void rk_or(unsigned* p, unsigned v) { atomicOr(p, v); }
__device__ __forceinline__ int rk_load_lds(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
// a cell other workgroups update in this launch: past this CU's L1.  What it returns may be old; see box_min / box_max.
__device__ __forceinline__ long long rk_load_global64(const int64_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void rk_min32(int* p, int v) { atomicMin(p, v); }
__device__ __forceinline__ void rk_max32(int* p, int v) { atomicMax(p, v); }
// (the fields these two touch are never negative)
__device__ __forceinline__ void rk_min64(int64_t* p, long long v) { atomicMin((unsigned long long*)p, (unsigned long long)v); }
__device__ __forceinline__ void rk_max64(int64_t* p, long long v) { atomicMax((unsigned long long*)p, (unsigned long long)v); }
__device__ __forceinline__ unsigned long long rk_ballot_prev(int pred, int v, int* prev) {
  const int up = __shfl_up(v, 1, 64);
  *prev = (threadIdx.x & 63) ? up : v;
  return __ballot(pred);
}
__device__ __forceinline__ unsigned long long rk_ballot(int pred) { return __ballot(pred); }
#endif

__device__ __forceinline__ void add64(int64_t* p, long long v) { atomicAdd((unsigned long long*)p, (unsigned long long)v); }

// A box edge only ever moves outwards, so an OLD value that already covers v proves that the current one does: the read saves
// the atomic for every tile in the interior of a large component, and nothing is lost when it is stale the other way.
__device__ __forceinline__ void box_min(int64_t* p, long long v) { if (v < rk_load_global64(p)) rk_min64(p, v); }
__device__ __forceinline__ void box_max(int64_t* p, long long v) { if (v > rk_load_global64(p)) rk_max64(p, v); }

__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// exclusive prefix of v over the workgroup's kNT threads (Hillis-Steele in LDS); *total = the sum.  s may be reused afterwards.
__device__ __forceinline__ int block_exclusive_scan(int v, int* s, int* total) {
  const int t = threadIdx.x;
  s[t] = v;
  __syncthreads();
#pragma unroll
  for (int off = 1; off < kNT; off <<= 1) {
    const int add = t >= off ? s[t - off] : 0;
    __syncthreads();
    s[t] += add;
    __syncthreads();
  }
  const int incl = s[t];
  *total = s[kNT - 1];
  __syncthreads();
  return incl - v;
}

struct RankArgs {
  int D, H, W;
  int ntx, nty, ntiles;      // tiles of (d) along x and y, and in all
  int n;                     // D * H * W < 2^31 - 1
  int nchunks, cap;
};

// (a) any order will do for a count: thread t takes the voxels t, t + 256, ... of the chunk, a wave 64 consecutive dwords per load
__global__ void __launch_bounds__(kNT)
k_rank_count(const int* __restrict__ labels, int* __restrict__ chunk, int n) {
  __shared__ int red[kWaves];
  const long long base = (long long)blockIdx.x * kChunk + threadIdx.x;
  int c = 0;
#pragma unroll
  for (int k = 0; k < kPerThread; ++k) {
    const long long i = base + k * kNT;
    c += i < n && labels[i] == (int)i + 1;
  }
  c = wave_sum_i(c);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    int s = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) s += red[w];
    chunk[blockIdx.x] = s;
  }
}

// (b) one workgroup; the table has been zeroed by the entry
__global__ void __launch_bounds__(kScanNT)
k_rank_scan(int* __restrict__ chunk, int64_t* __restrict__ count, int64_t* __restrict__ table, RankArgs a) {
  __shared__ int s[kScanNT];
  const int t = threadIdx.x;
  int carry = 0;
  for (int c0 = 0; c0 < a.nchunks; c0 += kScanNT) {   // (the same trip count in every thread)
    const int c = c0 + t;
    const int v = c < a.nchunks ? chunk[c] : 0;
    int total;
    const int ex = block_exclusive_scan(v, s, &total);
    if (c < a.nchunks) chunk[c] = carry + ex;
    carry += total;
  }
  if (t == 0) {
    count[0] = carry;
    count[1] = carry > a.cap ? carry - a.cap : 0;
    int64_t* bg = table;
    bg[0] = -1; bg[1] = a.n; bg[2] = 0; bg[3] = 0; bg[4] = 0; bg[5] = a.D; bg[6] = a.H; bg[7] = a.W; bg[8] = 0;
    if (carry > a.cap) {                              // the overflow row: an empty box that (d) widens
      int64_t* ov = table + (long long)(a.cap + 1) * kF;
      ov[0] = -1; ov[1] = 0; ov[2] = a.D; ov[3] = a.H; ov[4] = a.W; ov[5] = 0; ov[6] = 0; ov[7] = 0; ov[8] = -1;
    }
  }
}

// (c) the k-th root of the chunk, in index order, has rank chunk[blockIdx.x] + k + 1.  A wave owns a quarter of the chunk and
// reads it as kPerThread groups of 64 consecutive voxels; a ballot per group says which lanes hold a root, so a root's place
// within the wave is the roots of the groups before plus the roots of the lanes before it.  One barrier: the waves' totals.
__global__ void __launch_bounds__(kNT)
k_rank_roots(const uint8_t* __restrict__ pred, const int* __restrict__ labels, const int* __restrict__ chunk, int* __restrict__ ranks,
             int64_t* __restrict__ table, RankArgs a) {
  __shared__ int wave_total[kWaves];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long base = (long long)blockIdx.x * kChunk + wave * (kChunk / kWaves) + lane;
  const unsigned long long below = (1ull << lane) - 1;
  int place[kPerThread];                              // (every index is a constant once the loops are unrolled: registers)
  unsigned mine = 0;
  int run = 0;
#pragma unroll
  for (int g = 0; g < kPerThread; ++g) {
    const long long i = base + g * 64;
    const int root = i < a.n && labels[i] == (int)i + 1;
    const unsigned long long m = rk_ballot(root);
    place[g] = run + __builtin_popcountll(m & below);
    mine |= (unsigned)root << g;
    run += __builtin_popcountll(m);
  }
  if (lane == 0) wave_total[wave] = run;
  __syncthreads();
  int first = chunk[blockIdx.x];
  for (int w = 0; w < wave; ++w) first += wave_total[w];
#pragma unroll
  for (int g = 0; g < kPerThread; ++g) {
    if (!(mine >> g & 1)) continue;
    const long long i = base + g * 64;
    const int r = first + place[g] + 1;
    ranks[i] = r;
    if (r <= a.cap) {                                 // an empty box that (d) widens
      int64_t* row = table + (long long)r * kF;
      row[0] = i; row[1] = 0; row[2] = a.D; row[3] = a.H; row[4] = a.W; row[5] = 0; row[6] = 0; row[7] = 0; row[8] = pred[i];
    }
  }
}

// (d) one workgroup per tile.  Thread t owns column lx = t % 64 of the rows t / 64 + 4 j and adds a whole run of equal labels at
// once.  A slot's key goes from 0 to a label once and never changes again, so an insert finds its key or a free slot: there are
// as many slots as voxels.  A root's cell of ranks holds its rank since (c) and is only read here; every other cell is only
// written.
__global__ void __launch_bounds__(kNT)
k_rank_assign(const int* __restrict__ labels, int* ranks, int64_t* table, RankArgs a) {
  __shared__ int key[kTile];
  __shared__ int cnt[kTile];
  __shared__ unsigned zy[kTile], xlo[kTile], xhi[kTile];
  __shared__ int fg[kWaves];
  __shared__ int over[7];                             // the tile's share of the overflow row: voxels, box minima, box maxima
  const int t = threadIdx.x, lx = t & (kTX - 1), r0 = t / kTX;
  const unsigned mylo = lx < 32 ? 1u << lx : 0u, myhi = lx < 32 ? 0u : 1u << (lx - 32);
  int nfg = 0;
  if (t < 7) over[t] = t >= 1 && t <= 3 ? 0x7fffffff : 0;
  // A workgroup takes every gridDim.x-th tile: what all tiles add to ONE address -- the background's count, the overflow row --
  // is carried from tile to tile and reaches global memory once per workgroup.  (A thread zeroes the slots it has just flushed.)
  for (int tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
  const int tx = tile % a.ntx, rest = tile / a.ntx;
  const int ty = rest % a.nty, tz = rest / a.nty;
  const int x0 = tx * kTX, y0 = ty * kTY, z0 = tz * kTZ, x = x0 + lx;
  for (int s = t; s < kTile; s += kNT) { key[s] = 0; cnt[s] = 0; zy[s] = 0; xlo[s] = 0; xhi[s] = 0; }
  __syncthreads();
  int run_key = 0, run_n = 0, run_rank = 0;
  unsigned run_zy = 0;
  for (int j = 0; j <= kRowsPerThread; ++j) {
    int lab = 0;
    long long i = 0;
    unsigned bits = 0;
    if (j < kRowsPerThread) {
      const int row = r0 + j * kWaves, ly = row % kTY, lz = row / kTY;
      const int y = y0 + ly, z = z0 + lz;
      if (x < a.W && y < a.H && z < a.D) {
        i = ((long long)z * a.H + y) * a.W + x;
        lab = labels[i];
        bits = 1u << lz | 1u << (kTZ + ly);
        if (lab == 0) ranks[i] = 0;
      }
    }
    if (lab != run_key) {
      if (run_key != 0) {
        unsigned h = ((unsigned)run_key * 2654435761u) >> kHashShift;
        for (int probe = 0; probe < kTile; ++probe) {
          int k = rk_load_lds(&key[h]);
          if (k == 0) k = rk_cas(&key[h], 0, run_key);
          if (k == 0 || k == run_key) break;
          h = (h + 1) & (kTile - 1);
        }
        atomicAdd(&cnt[h], run_n);
        rk_or(&zy[h], run_zy);
        if (mylo) rk_or(&xlo[h], mylo);
        if (myhi) rk_or(&xhi[h], myhi);
        nfg += run_n;
      }
      run_key = lab;
      run_n = 0;
      run_zy = 0;
      if (lab != 0) run_rank = ranks[lab - 1];
    }
    if (lab != 0) {
      ++run_n;
      run_zy |= bits;
      if (lab != (int)i + 1) ranks[i] = run_rank;
    }
  }
  __syncthreads();                                    // every run of the tile is in the table
  for (int s = t; s < kTile; s += kNT) {
    if (key[s] == 0) continue;
    const int r = ranks[key[s] - 1];
    const unsigned zm = zy[s] & ((1u << kTZ) - 1), ym = zy[s] >> kTZ;
    const unsigned long long xm = (unsigned long long)xhi[s] << 32 | xlo[s];
    const int bz0 = z0 + __builtin_ctz(zm), by0 = y0 + __builtin_ctz(ym), bx0 = x0 + __builtin_ctzll(xm);
    const int bz1 = z0 + 32 - __builtin_clz(zm), by1 = y0 + 32 - __builtin_clz(ym), bx1 = x0 + 64 - __builtin_clzll(xm);
    if (r > a.cap) {                                  // thousands of specks share this one row: gathered per tile first
      atomicAdd(&over[0], cnt[s]);
      rk_min32(&over[1], bz0); rk_min32(&over[2], by0); rk_min32(&over[3], bx0);
      rk_max32(&over[4], bz1); rk_max32(&over[5], by1); rk_max32(&over[6], bx1);
      continue;
    }
    int64_t* row = table + (long long)r * kF;
    add64(row + 1, cnt[s]);
    box_min(row + 2, bz0); box_min(row + 3, by0); box_min(row + 4, bx0);
    box_max(row + 5, bz1); box_max(row + 6, by1); box_max(row + 7, bx1);
  }
  }
  nfg = wave_sum_i(nfg);
  if ((t & 63) == 0) fg[t >> 6] = nfg;
  __syncthreads();
  if (t == 0) {                                       // the background row starts at n: one subtraction per workgroup
    int s = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) s += fg[w];
    if (s) add64(table + 1, -(long long)s);
  }
  if (t == 0 && over[0] != 0) {
    int64_t* row = table + (long long)(a.cap + 1) * kF;
    add64(row + 1, over[0]);
    box_min(row + 2, over[1]); box_min(row + 3, over[2]); box_min(row + 4, over[3]);
    box_max(row + 5, over[4]); box_max(row + 6, over[5]); box_max(row + 7, over[6]);
  }
}

struct OverlapArgs {
  int n;                     // D * H * W
  int capa, capb;            // the clamps: cap_a + 1, cap_b + 1
  int steps;                 // steps of kStep voxels per workgroup
};

// (e)
__global__ void __launch_bounds__(kNT)
k_rank_overlap(const int* __restrict__ va, const int* __restrict__ vb, int64_t* overlap, OverlapArgs a) {
  __shared__ int key[kPairSlots];
  __shared__ int cnt[kPairSlots];
  __shared__ int bgs[kWaves];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  for (int s = t; s < kPairSlots; s += kNT) { key[s] = 0; cnt[s] = 0; }
  __syncthreads();
  const int nb = a.capb + 1;                          // cells per row
  const long long first = (long long)blockIdx.x * a.steps * kStep;
  int bg = 0;
  for (int st = 0; st < a.steps; ++st) {
    const long long base = first + (long long)st * kStep + wave * (64 * kU) + lane;
    if (base - lane >= a.n) break;                    // (wave-uniform)
    int ra[kU], rb[kU];
#pragma unroll
    for (int u = 0; u < kU; ++u) {
      const long long i = base + u * 64;
      const long long j = i < a.n ? i : a.n - 1;
      ra[u] = va[j];
      rb[u] = vb[j];
    }
#pragma unroll
    for (int u = 0; u < kU; ++u) {
      const bool valid = base + u * 64 < a.n;
      const int ia = (unsigned)ra[u] < (unsigned)a.capa ? ra[u] : a.capa;
      const int ib = (unsigned)rb[u] < (unsigned)a.capb ? rb[u] : a.capb;
      const int cell = valid ? ia * nb + ib : -1;     // 0: both backgrounds; -1: past the end, counts nothing
      bg += cell == 0;
      int prev;
      const unsigned long long some = rk_ballot_prev(cell > 0, cell, &prev);
      if (some == 0) continue;                        // (wave-uniform) nothing but background: the usual case
      const bool changed = lane == 0 || cell != prev;
      const unsigned long long edges = rk_ballot(changed);
      if (cell > 0 && changed) {                      // the first lane of a run: its length is the distance to the next edge
        const unsigned long long above = lane == 63 ? 0ull : edges >> (lane + 1);
        const int len = above ? __builtin_ctzll(above) + 1 : 64 - lane;
        unsigned h = ((unsigned)cell * 2654435761u) >> kHashShift;
        bool placed = false;
        for (int probe = 0; probe < kMaxProbe; ++probe) {
          int k = rk_load_lds(&key[h]);
          if (k == 0) k = rk_cas(&key[h], 0, cell);
          if (k == 0 || k == cell) { placed = true; break; }
          h = (h + 1) & (kPairSlots - 1);
        }
        if (placed) atomicAdd(&cnt[h], len);
        else add64(overlap + cell, len);
      }
    }
  }
  bg = wave_sum_i(bg);
  if (lane == 0) bgs[wave] = bg;
  __syncthreads();
  if (t == 0) {
    long long s = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) s += bgs[w];
    if (s) add64(overlap, s);
  }
  for (int s = t; s < kPairSlots; s += kNT)
    if (key[s] != 0) add64(overlap + key[s], cnt[s]);
}

bool dims_ok(int D, int H, int W) {
  if (D < 0 || H < 0 || W < 0) return false;
  if (D == 0 || H == 0 || W == 0) return true;
  const long long lim = (1ll << 31) - 1, dh = (long long)D * H;
  return dh < lim && dh * W < lim;
}

bool cap_ok(int cap) { return cap >= 1 && cap <= CFUN_LESION_MAX_CAP; }

long long chunks_of(long long n) { return (n + kChunk - 1) / kChunk; }

}  // namespace

extern "C" size_t cfun_lesion_workspace_bytes(int32_t D, int32_t H, int32_t W, int32_t cap) {
  if (!dims_ok(D, H, W) || !cap_ok(cap) || D == 0 || H == 0 || W == 0) return 0;
  return (size_t)chunks_of((long long)D * H * W) * sizeof(int);
}

extern "C" int cfun_cc_rank(const uint8_t* pred, const int32_t* labels, const int32_t* dims, int32_t cap, int32_t* ranks,
                            int64_t* count, int64_t* table, void* workspace, size_t workspace_bytes, cfun_stream_t stream) {
  if (!dims || !count || !table || !cap_ok(cap)) return CFUN_EINVAL;
  if (!dims_ok(dims[0], dims[1], dims[2])) return CFUN_EINVAL;
  hipStream_t st = cfun_st(stream);
  const size_t table_bytes = (size_t)(cap + 2) * kF * sizeof(int64_t);
  if (dims[0] == 0 || dims[1] == 0 || dims[2] == 0) {
    if (hipMemsetAsync(count, 0, 2 * sizeof(int64_t), st) != hipSuccess) return CFUN_EINVAL;
    if (hipMemsetAsync(table, 0, table_bytes, st) != hipSuccess) return CFUN_EINVAL;
    return CFUN_OK;
  }
  if (!pred || !labels || !ranks) return CFUN_EINVAL;
  RankArgs a;
  a.D = dims[0]; a.H = dims[1]; a.W = dims[2];
  a.ntx = (int)(((long long)a.W + kTX - 1) / kTX);    // (a dimension may be close to 2^31)
  a.nty = (int)(((long long)a.H + kTY - 1) / kTY);
  a.n = (int)((long long)a.D * a.H * a.W);
  a.nchunks = (int)chunks_of(a.n);
  a.cap = cap;
  if (!workspace || workspace_bytes < cfun_lesion_workspace_bytes(a.D, a.H, a.W, cap)) return CFUN_EWORKSPACE;
  int* chunk = (int*)workspace;
  a.ntiles = (int)((((long long)a.D + kTZ - 1) / kTZ) * a.nty * a.ntx);        // (< 2^31 voxels: far fewer tiles)
  if (hipMemsetAsync(table, 0, table_bytes, st) != hipSuccess) return CFUN_EINVAL;
  hipLaunchKernelGGL(k_rank_count, dim3((unsigned)a.nchunks), dim3(kNT), 0, st, labels, chunk, a.n);
  CFUN_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_rank_scan, dim3(1), dim3(kScanNT), 0, st, chunk, count, table, a);
  CFUN_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_rank_roots, dim3((unsigned)a.nchunks), dim3(kNT), 0, st, pred, labels, (const int*)chunk, ranks, table, a);
  CFUN_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_rank_assign, dim3((unsigned)(a.ntiles < kAssignWG ? a.ntiles : kAssignWG)), dim3(kNT), 0, st, labels, ranks, table, a);
  CFUN_LAUNCH_CHECK();
  return CFUN_OK;
}

extern "C" int cfun_rank_overlap(const int32_t* va, const int32_t* vb, const int32_t* dims, int32_t cap_a, int32_t cap_b,
                                 int64_t* overlap, void* workspace, size_t workspace_bytes, cfun_stream_t stream) {
  (void)workspace; (void)workspace_bytes;
  if (!dims || !overlap || !cap_ok(cap_a) || !cap_ok(cap_b)) return CFUN_EINVAL;
  if (!dims_ok(dims[0], dims[1], dims[2])) return CFUN_EINVAL;
  hipStream_t st = cfun_st(stream);
  const bool empty = dims[0] == 0 || dims[1] == 0 || dims[2] == 0;
  if (!empty && (!va || !vb)) return CFUN_EINVAL;
  if (hipMemsetAsync(overlap, 0, (size_t)(cap_a + 2) * (cap_b + 2) * sizeof(int64_t), st) != hipSuccess) return CFUN_EINVAL;
  if (empty) return CFUN_OK;
  OverlapArgs a;
  a.n = (int)((long long)dims[0] * dims[1] * dims[2]);
  a.capa = cap_a + 1;
  a.capb = cap_b + 1;
  const long long nsteps = ((long long)a.n + kStep - 1) / kStep;
  long long nwg = (nsteps + kMinSteps - 1) / kMinSteps;
  if (nwg > kMaxWG) nwg = kMaxWG;
  a.steps = (int)((nsteps + nwg - 1) / nwg);
  nwg = (nsteps + a.steps - 1) / a.steps;             // (no workgroup without a step)
  hipLaunchKernelGGL(k_rank_overlap, dim3((unsigned)nwg), dim3(kNT), 0, st, va, vb, overlap, a);
  CFUN_LAUNCH_CHECK();
  return CFUN_OK;
}
