// The lock-free union-find forest of the connected-component kernels (cc.hip) and of the hole filling built on it (fill.hip):
// the atomics with their CFUN_HIP_EMULATION stand-ins, the two homes of a forest (LDS, global), find() and unite().
//
// The forest.  A cell holds the index of its voxel's parent (LDS) or 1 + that index (global: 0 stays free for "no voxel"), and a
// parent's index is never larger than the child's; a root holds its own index.  Links only ever go from a larger root to a
// smaller index, so a tree's root is the smallest index in it, and once every adjacency has been united the root of a voxel is
// the smallest index of its component: the canonical label.
//
// Workgroups talk only through integer atomics on global memory and through kernel boundaries.  No workgroup waits for another:
// there is no flag, no ticket, no spin on a value someone else must write, and every loop below ends by itself (see unite()).
#ifndef CFUN_CC_FOREST_H
#define CFUN_CC_FOREST_H

#include "common.h"

namespace {

// ---- atomics.  tests/emu/hip/hip_runtime.h has atomicAdd only; its fibers switch at rendezvous points only and its workgroups
// run one after another, so a plain read-modify-write is atomic there.
#ifdef CFUN_HIP_EMULATION
__device__ __forceinline__ int cc_min(int* p, int v) { const int o = *p; if (v < o) *p = v; return o; }
__device__ __forceinline__ unsigned long long cc_max64(unsigned long long* p, unsigned long long v) {
  const unsigned long long o = *p; if (v > o) *p = v; return o;
}
__device__ __forceinline__ int cc_cas(int* p, int expect, int v) { const int o = *p; if (o == expect) *p = v; return o; }
__device__ __forceinline__ int cc_load_global(const int* p) { return *p; }
__device__ __forceinline__ int cc_load_lds(const int* p) { return *p; }
#else
__device__ __forceinline__ int cc_min(int* p, int v) { return atomicMin(p, v); }                 // relaxed, agent scope
__device__ __forceinline__ unsigned long long cc_max64(unsigned long long* p, unsigned long long v) { return atomicMax(p, v); }
__device__ __forceinline__ int cc_cas(int* p, int expect, int v) { return atomicCAS(p, expect, v); }
// A cell another workgroup may update in this launch: a relaxed agent-scope load goes past this CU's L1, which no other CU's
// atomic ever refreshes.  What it returns may still be old (the L2s of the XCDs are not coherent with each other); unite() does
// not need it fresh.
__device__ __forceinline__ int cc_load_global(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ int cc_load_lds(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
#endif

// The forest lives either in LDS (cells hold the parent's tile-local index) or in the labels array (cells hold 1 + the parent's
// global index: 0 stays free for "no voxel").
struct LdsForest {
  int* cell;
  __device__ __forceinline__ int parent(int i) const { return cc_load_lds(cell + i); }
  __device__ __forceinline__ int link(int i, int to) const { return cc_min(cell + i, to); }
};
struct GlobalForest {
  int* cell;
  __device__ __forceinline__ int parent(int i) const { return cc_load_global(cell + i) - 1; }
  __device__ __forceinline__ int link(int i, int to) const { return cc_min(cell + i, to + 1) - 1; }
};

// Every value a cell has ever held is the index of a member of the cell's own set, and never larger than the cell's index; so a
// read that returns an OLD value of a cell still yields a member of the same set, at or below the cell: the walk goes strictly
// down and ends at an index that read as its own parent.  That index need not be a root any more; unite() finds out.
template <class F>
__device__ __forceinline__ int find(const F& f, int i) {
  for (;;) {
    const int p = f.parent(i);
    if (p == i) return i;
    i = p;
  }
}

// Unite the sets of two adjacent voxels.  Lock-free: nothing here waits for a value another thread must write.
//   * The only write is link(a, b) = atomic-min of cell a with b, for a > b.  Its RETURN VALUE, not any load, says what happened:
//     the atomic is performed at the one place that holds the cell, whatever a cache showed before.
//   * It returned a: a was a root at that instant and now hangs under b.  Done.
//   * It returned old < a: a was not a root (a stale read made it look like one, or another thread linked it first).  If b < old
//     the min has replaced a's parent old by b, which cuts a off old; either way what remains to be done is unite(old, b), and
//     the loop goes on with exactly that.  Nothing is lost: a -> min(old, b), and old and b get united.
//   * Termination: the larger of the two indices strictly decreases every round (old < a and b < a, and find() only goes down);
//     both are >= 0.  No round depends on another thread making progress.
// At the end of the launch every adjacency has passed through here, so every tree is a whole component, its root the smallest
// index in it.  Integer min is commutative and associative: the forest's SHAPE depends on the schedule, the roots do not.
template <class F>
__device__ __forceinline__ void unite(const F& f, int a, int b) {
  a = find(f, a);
  b = find(f, b);
  while (a != b) {
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = f.link(a, b);
    if (old == a) return;
    a = find(f, old);
    b = find(f, b);
  }
}

// k = 0 .. 12 -> the backward half of the 3 x 3 x 3 neighbourhood (the neighbours with a smaller linear index); faces: k = 4, 10, 12
__device__ __forceinline__ void backward_offset(int k, int& dz, int& dy, int& dx) {
  if (k < 9) { dz = -1; dy = k / 3 - 1; dx = k % 3 - 1; }
  else if (k < 12) { dz = 0; dy = -1; dx = k - 10; }
  else { dz = 0; dy = 0; dx = -1; }
}
__device__ __forceinline__ bool is_face(int k) { return k == 4 || k == 10 || k == 12; }

}  // namespace

#endif
