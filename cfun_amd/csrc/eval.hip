// Segmentation scoring on the device (include/cfun_eval.h): the (K+1) x (K+1) confusion counts of a predicted class map against a
// label volume -- everything the reference's compute_per_class_mask_iou / compute_mask_iou (utils.py:580-617) are a function of,
// without its two float64 one-hot arrays.
//   (a) k_confusion_tiled    label with z (or y) fastest (the loader's [H,W,D] array read in place), pred [D,H,W] with x fastest
//   (b) k_confusion_straight any other stride set: a flat sweep in pred's order that indexes the label through its strides
//   (c) k_confusion_finish   per-workgroup uint32 partials -> int64 counts, one workgroup per bin
// No global atomics and no float atomics: the only atomics are integer adds on a per-wave LDS histogram, the partials are summed
// as integers, so every run gives the same bits.
//
// Tile of (a): a workgroup takes one row y, 128 x, 128 z.  (A label whose unit-stride axis is y -- the same [H,W,D] array in Fortran
// order, which is how a NIfTI file is laid out -- runs the same kernel with the roles of y and z exchanged; "z" below is that axis.)
// Pass 1: every wave reads rows of pred along x -- 128 consecutive bytes = one line's worth, as two 64-lane byte loads issued back
// to back -- and stores them as COLUMNS of a [128 x][132 B] LDS tile.
// ds_write_b8 at byte address x * 132 + z: the dword index is x * 33 + z / 4, so the 64 lanes of a store (consecutive x, one z)
// fall on 64 distinct banks of the 64.  Pass 2: per (y, x) the wave reads the label's run along z (128 elements: 512 B of int32 or
// 128 B of uint8, again two loads) and the matching 128 bytes of the tile row x (consecutive bytes: 16 dwords per load, no
// conflict).  The byte-wide pred is the side that is turned: the tile costs 16.5 KiB where an int32 tile would cost 66 KiB.
//
// Counting: well over 90 % of a CT volume is the pair (label 0, pred 0).  Those are counted in a register per thread and summed
// once per wave with shuffles; only the other pairs go to the wave's own LDS histogram with an integer atomicAdd, and of those a
// thread adds a whole run of equal pairs at once (count_pair).  A workgroup
// loops over tiles (the grid is capped at kMaxWG workgroups) and writes its (K+1)^2 sums once, bin-major, so that the finish
// launch reads each bin's partials as one coalesced run.
#include "common.h"
#include "../../include/cfun_eval.h"

namespace {

constexpr int kNT = 256, kWaves = kNT / 64;
constexpr int kTX = 128, kTQ = 128, kPitch = 132;     // bytes; 132 / 4 = 33 dwords: odd, so a column store is conflict-free
constexpr int kMaxBins = 256;                         // (K + 1)^2 with K <= 15
constexpr int kMaxWG = 1536;                          // workgroups per pass: 6 per CU of the MI355X's 256 (6 x 20.5 KiB of LDS, 24 waves)
constexpr int kBatch = 4;                             // label runs a wave loads before it counts the first
constexpr int kStraightPerWG = kNT * 16;              // voxels a workgroup of the straight path takes before the grid is capped

struct ConfArgs {
  long long sD, sH, sW;      // element strides of the label along z, y, x
  int D, H, W, K;
  // tiled path: q is the label's unit-stride axis (z, or y), r the remaining one; pred[q * pQ + r * pR + x], label[r * lR + x * lX + q]
  long long pQ, pR, lR, lX;
  int Q, R;
  int ntx, ntiles;           // tiles along x, in all
  int nwg;
};

template <typename L>
__device__ __forceinline__ int class_of(L v, int K) {
  const int i = (int)v;
  return (unsigned)i < (unsigned)K ? i : K;           // negative or >= K: the extra row / column K ("other")
}

__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// One voxel's pair.  (0,0) goes to the thread's background counter.  Any other pair extends the thread's current run when it is the
// same bin as the voxel before (a thread walks along x at a fixed z, so inside an organ it almost always is) and only a change of
// bin costs an LDS atomic: 64 lanes adding to one address would otherwise serialise exactly where the volume is not background.
struct Run { int bin, n, bg; };

__device__ __forceinline__ void count_pair(Run& r, int* __restrict__ hist, int g, int p, int nk) {
  const int bin = g * nk + p;
  if (bin == 0) { ++r.bg; return; }
  if (bin == r.bin) { ++r.n; return; }
  if (r.n) atomicAdd(&hist[r.bin], r.n);
  r.bin = bin;
  r.n = 1;
}

// the calling workgroup's per-wave histograms (+ the per-thread runs and background counts) -> partials[bin * nwg + wg]
__device__ __forceinline__ void write_partials(int (*hist)[kMaxBins], Run r, int nb, int nwg, uint32_t* __restrict__ partials) {
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  if (r.n) atomicAdd(&hist[wave][r.bin], r.n);
  const int bg = wave_sum_i(r.bg);
  if (lane == 0) hist[wave][0] = bg;                  // bin 0 = (0,0) never receives an atomic
  __syncthreads();
  if (t < nb) {
    unsigned s = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) s += (unsigned)hist[w][t];
    partials[(long long)t * nwg + blockIdx.x] = s;
  }
}

template <typename L>
__global__ void __launch_bounds__(kNT)
k_confusion_tiled(const uint8_t* __restrict__ pred, const L* __restrict__ lab, uint32_t* __restrict__ partials, ConfArgs a) {
  __shared__ uint8_t tile[kTX * kPitch];
  __shared__ int hist[kWaves][kMaxBins];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int nk = a.K + 1, nb = nk * nk;
  hist[wave][lane] = 0; hist[wave][lane + 64] = 0; hist[wave][lane + 128] = 0; hist[wave][lane + 192] = 0;
  Run run = {0, 0, 0};

  for (int tid = blockIdx.x; tid < a.ntiles; tid += a.nwg) {
    const int tx = tid % a.ntx, rest = tid / a.ntx;
    const int r = rest % a.R, tq = rest / a.R;
    const int x0 = tx * kTX, q0 = tq * kTQ;
    const int nx = a.W - x0 < kTX ? a.W - x0 : kTX, nq = a.Q - q0 < kTQ ? a.Q - q0 : kTQ;      // the tile's extent: both >= 1
    __syncthreads();                                  // (the previous tile's pass 2 has read the tile; hist is zeroed)
    // pass 1.  Lanes past the row's end re-read its last byte into tile columns that pass 2 never looks at: every load is
    // unconditional, so the compiler keeps a whole unrolled batch of them in flight.
    const long long pa = (long long)r * a.pR + x0 + (lane < nx ? lane : nx - 1);
    const long long pb = (long long)r * a.pR + x0 + (lane + 64 < nx ? lane + 64 : nx - 1);
#pragma unroll 8
    for (int qq = wave; qq < nq; qq += kWaves) {
      const long long row = (long long)(q0 + qq) * a.pQ;
      tile[lane * kPitch + qq] = pred[row + pa];
      tile[(lane + 64) * kPitch + qq] = pred[row + pb];
    }
    __syncthreads();
    // pass 2, four (y, x) runs of the label per step: eight loads are issued before the first pair is counted
    const bool va = lane < nq, vb = lane + 64 < nq;
    const long long la = (long long)r * a.lR + q0 + (va ? lane : nq - 1), lb = (long long)r * a.lR + q0 + (vb ? lane + 64 : nq - 1);
    for (int xi = wave; xi < nx; xi += kWaves * kBatch) {
      L ga[kBatch], gb[kBatch];
#pragma unroll
      for (int u = 0; u < kBatch; ++u) {
        const int xx = xi + u * kWaves < nx ? xi + u * kWaves : nx - 1;
        const long long base = (long long)(x0 + xx) * a.lX;
        ga[u] = lab[base + la];
        gb[u] = lab[base + lb];
      }
#pragma unroll
      for (int u = 0; u < kBatch; ++u) {
        const int xx = xi + u * kWaves;
        if (xx < nx) {                                // (wave-uniform)
          if (va) count_pair(run, hist[wave], class_of(ga[u], a.K), class_of(tile[xx * kPitch + lane], a.K), nk);
          if (vb) count_pair(run, hist[wave], class_of(gb[u], a.K), class_of(tile[xx * kPitch + lane + 64], a.K), nk);
        }
      }
    }
  }
  write_partials(hist, run, nb, a.nwg, partials);
}

template <typename L>
__global__ void __launch_bounds__(kNT)
k_confusion_straight(const uint8_t* __restrict__ pred, const L* __restrict__ lab, uint32_t* __restrict__ partials, ConfArgs a) {
  __shared__ int hist[kWaves][kMaxBins];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int nk = a.K + 1, nb = nk * nk;
  hist[wave][lane] = 0; hist[wave][lane + 64] = 0; hist[wave][lane + 128] = 0; hist[wave][lane + 192] = 0;
  Run run = {0, 0, 0};
  __syncthreads();
  const long long n = (long long)a.D * a.H * a.W;
  for (long long i = (long long)blockIdx.x * kNT + t; i < n; i += (long long)a.nwg * kNT) {
    const long long r = i / a.W;
    const int x = (int)(i - r * a.W), y = (int)(r % a.H), z = (int)(r / a.H);
    count_pair(run, hist[wave], class_of(lab[z * a.sD + y * a.sH + x * a.sW], a.K), class_of(pred[i], a.K), nk);
  }
  write_partials(hist, run, nb, a.nwg, partials);
}

// one workgroup per bin: its nwg partials are one coalesced run; integers, so the order of the sum does not matter
__global__ void __launch_bounds__(kNT)
k_confusion_finish(const uint32_t* __restrict__ partials, int nwg, int64_t* __restrict__ counts) {
  __shared__ long long red[kWaves];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, b = blockIdx.x;
  long long s = 0;
#pragma unroll 4
  for (int w = threadIdx.x; w < nwg; w += kNT) s += (long long)partials[(long long)b * nwg + w];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  if (lane == 0) red[wave] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    long long total = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) total += red[w];
    counts[b] = total;
  }
}

int cap_wg(long long n) { return (int)(n < kMaxWG ? n : kMaxWG); }

long long tiles_of(int Q, int R, int W) {
  return (long long)((W + kTX - 1) / kTX) * R * ((Q + kTQ - 1) / kTQ);
}

long long chunks_of(int D, int H, int W) {
  return ((long long)D * H * W + kStraightPerWG - 1) / kStraightPerWG;
}

bool dims_ok(int D, int H, int W, int K) {
  return D >= 0 && H >= 0 && W >= 0 && K >= 1 && K <= 15 && (D == 0 || H == 0 || W == 0 || (long long)D * H * W < (1ll << 31));
}

template <typename L>
void launch_pass(const uint8_t* pred, const void* label, uint32_t* partials, const ConfArgs& a, bool tiled, hipStream_t st) {
  if (tiled)
    hipLaunchKernelGGL(k_confusion_tiled<L>, dim3((unsigned)a.nwg), dim3(kNT), 0, st, pred, (const L*)label, partials, a);
  else
    hipLaunchKernelGGL(k_confusion_straight<L>, dim3((unsigned)a.nwg), dim3(kNT), 0, st, pred, (const L*)label, partials, a);
}

}  // namespace

extern "C" size_t cfun_seg_confusion_workspace_bytes(int32_t D, int32_t H, int32_t W, int32_t K) {
  if (!dims_ok(D, H, W, K) || D == 0 || H == 0 || W == 0) return 0;
  long long n = chunks_of(D, H, W);                    // the largest grid of the three paths: the strides are not known here
  if (tiles_of(D, H, W) > n) n = tiles_of(D, H, W);
  if (tiles_of(H, D, W) > n) n = tiles_of(H, D, W);
  return (size_t)cap_wg(n) * (size_t)((K + 1) * (K + 1)) * sizeof(uint32_t);
}

extern "C" int cfun_seg_confusion(const uint8_t* pred, const void* label, int32_t label_dtype, const int64_t* label_strides,
                                  const int32_t* dims, int32_t K, int64_t* counts, void* workspace, size_t workspace_bytes,
                                  cfun_stream_t stream) {
  if (!dims || !label_strides || !counts || (label_dtype != 0 && label_dtype != 1)) return CFUN_EINVAL;
  ConfArgs a;
  a.D = dims[0]; a.H = dims[1]; a.W = dims[2]; a.K = K;
  if (!dims_ok(a.D, a.H, a.W, K)) return CFUN_EINVAL;
  const int nb = (K + 1) * (K + 1);
  hipStream_t st = cfun_st(stream);
  if (a.D == 0 || a.H == 0 || a.W == 0) {              // nothing to count: the finish launch alone writes the zeros
    hipLaunchKernelGGL(k_confusion_finish, dim3((unsigned)nb), dim3(kNT), 0, st, (const uint32_t*)workspace, 0, counts);
    CFUN_LAUNCH_CHECK();
    return CFUN_OK;
  }
  if (!pred || !label) return CFUN_EINVAL;
  a.sD = label_strides[0]; a.sH = label_strides[1]; a.sW = label_strides[2];
  const bool tiled = a.sD == 1 || a.sH == 1;
  if (a.sD == 1) {                                     // z fastest: the loader's [H,W,D] array in C order
    a.Q = a.D; a.R = a.H; a.pQ = (long long)a.H * a.W; a.pR = a.W; a.lR = a.sH;
  } else {                                             // y fastest: the same array in Fortran order, as a NIfTI file stores it
    a.Q = a.H; a.R = a.D; a.pQ = a.W; a.pR = (long long)a.H * a.W; a.lR = a.sD;
  }
  a.lX = a.sW;
  a.ntx = (a.W + kTX - 1) / kTX;
  const long long tiles = tiles_of(a.Q, a.R, a.W);
  a.ntiles = (int)tiles;                               // < 2^31 voxels: far fewer tiles
  a.nwg = cap_wg(tiled ? tiles : chunks_of(a.D, a.H, a.W));
  if (!workspace || workspace_bytes < (size_t)a.nwg * nb * sizeof(uint32_t)) return CFUN_EWORKSPACE;
  uint32_t* partials = (uint32_t*)workspace;
  if (label_dtype == 0) launch_pass<uint8_t>(pred, label, partials, a, tiled, st);
  else launch_pass<int32_t>(pred, label, partials, a, tiled, st);
  CFUN_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_confusion_finish, dim3((unsigned)nb), dim3(kNT), 0, st, (const uint32_t*)partials, a.nwg, counts);
  CFUN_LAUNCH_CHECK();
  return CFUN_OK;
}
