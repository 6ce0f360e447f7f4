// The stream-K "relay" of the B-streamed persistent GEMMs (conv_bstream.hip: fp32 MFMA, conv_bxs.hip: bf16x3 emulation):
// the place the protocol is described and most of it lives -- the library's only synchronisation between workgroups.
// Device side: relay_split, relay_load_head, relay_park_head and the load streams' position (RelayPos).  Host side: the
// workspace size, the grid rule and the launch-time check of the error word (defined in conv_bstream.hip).  Still written out in EACH kernel, and to be changed
// in both together: the flag pointer, the epoch load, launch_done (ticket + launch counter) and seg_of (see below why); the
// two-line wrappers pos_init / pos_next over RelayPos sit beside seg_of.
//
// Work split (a stream-K that keeps the accumulation order): the launch is T tiles x `nit` iterations of 128 k;
// workgroup w (numbered so that one XCD holds consecutive w) takes the units [U w / G, U (w+1) / G) of that linear
// space, so every CU gets the same number of MFMAs whatever T is -- no partial last round (M = 16 800 / 67 200 pixels
// at layer4 / layer3: 528 or 1050 tiles on 256 CUs lost 31 % / 18 % to it).  A range that ends inside a tile computes
// the tile's HEAD k range and parks the 128 x 128 accumulators in the workspace (64 KB per workgroup); the next
// workgroup, whose range starts inside that tile, loads them and CONTINUES the same k chain before the epilogue --
// the sum is the sequential one, bit for bit.  Order inside a workgroup: head first, whole tiles, tail last; with at
// least one tile of work per workgroup (the host checks: relay_workspace) the head of w-1 is finished before the tail
// of w starts, so the flag wait never spins in practice and cannot deadlock (the writer waits for nobody).  Without a
// workspace the tiles go round-robin (no relay).
//
// Bookkeeping behind the accumulator sets: [G] flags, launch counter, finished-workgroup ticket.
// A flag carries the EPOCH of the launch that raised it (counter + 1), never 0 / 1: a reader waits for exactly this
// launch's value and nobody resets anything, so a writer that arrives after its reader gave up (see the time-out in
// load_head) cannot leave a flag that a later launch on this workspace would mistake for its own.  The counter is
// advanced by the last workgroup to finish; every workgroup reads it before it takes its ticket, so all G see one value.
// Both kernels keep this one layout: a workspace zero-filled once serves launches of either, in any order.
#pragma once
#include "common.h"

namespace hnd {

// ---- host side
// tiles of a launch with `wn` wave columns (block tile 64 * 4 / wn x 64 * wn) and the persistent grid
inline void relay_grid(const hnd_conv_desc& d, int wn, int& mtiles, int& ntiles, int& grid) {
  const int bm = 64 * (4 / wn), bn = 64 * wn;
  mtiles = (int)((gemm_rows(d) + bm - 1) / bm);
  ntiles = d.cout / bn;
  grid = (cu_count() / 8) * 8;
}
constexpr int RELAY_THREADS = 256, RELAY_SET = 16 * RELAY_THREADS * 4;     // threads of a workgroup, floats it parks
// accumulator sets, flags, counter + ticket
inline size_t relay_workspace_bytes(int grid) { return (size_t)grid * (RELAY_SET * sizeof(float) + sizeof(int)) + 16 * sizeof(int); }
// ... of the launch of `d` with `wn` wave columns (0: not taken); 0 without one whole tile of work per workgroup (see above)
inline size_t relay_workspace(const hnd_conv_desc& d, int wn) {
  if (wn == 0) return 0;
  int mtiles, ntiles, grid;
  relay_grid(d, wn, mtiles, ntiles, grid);
  if ((long long)mtiles * ntiles < grid) return 0;
  return relay_workspace_bytes(grid);
}
// Launch-time side of the time-out: while the sticky error word is raised no launch is made (HND_ERR_LAUNCH, the message
// names `kernel`); else fills in the bound of the flag wait (HND_BSTREAM_SPIN) and the device view of the word.
int relay_launch_check(const char* kernel, int& spin_limit, int*& err);
// the error word: raised (1) or not, optionally acknowledged (hnd_relay_timeouts)
int relay_timeouts(int reset);

// ---- device side: the pieces both kernels call.  They are free functions over the kernels' OWN locals and argument struct,
// not a struct with state: bstream_kernel and bxs_kernel run at the register limit, and hipcc's allocation changed as soon
// as the split went through an aggregate or spin_limit / err were copied at the top of the kernel (NOTEBOOK section 15).
// With these signatures every instantiation compiles to the parent's instruction stream.  What stays in each kernel, a few
// lines each and commented there: the flag pointer, the epoch load, launch_done and seg_of.  (launch_done as a shared
// function over (relay, relay_f, G, epoch, tid) was tried and moved instructions in all 16 instantiations: NOTEBOOK
// section 18.)
// Fixed geometry, on both sides: workgroups of RELAY_THREADS threads, each parking its 4 x 4 f32x4 accumulators (a 128 x 128
// or 256 x 64 tile) = RELAY_SET floats per workgroup.

// This workgroup's share: the units [U lb / G, U (lb + 1) / G) of T tiles x nit iterations as a head (has_head: tile tB,
// iterations [0, offB)), nfull whole tiles from first_full and a tail (offA > 0: tile tA, iterations [offA, nit)); without a
// workspace the tiles lb, lb + G, ...  False: nothing to do and no bookkeeping either (no workspace, lb >= T).
// `nit` by reference ON PURPOSE: by value, hipcc allocates the kernels' registers differently (as with Args above).
__device__ __forceinline__ bool relay_split(const float* relay, int lb, int G, int T, const int& nit, int& nseg, int& first_full,
                                            int& nfull, int& tA, int& offA, int& tB, int& offB, bool& has_head) {
  if (relay) {
    const long long U = (long long)T * nit;
    const long long u0 = U * lb / G, u1 = U * (lb + 1) / G;
    tA = (int)(u0 / nit); offA = (int)(u0 - (long long)tA * nit);
    tB = (int)(u1 / nit); offB = (int)(u1 - (long long)tB * nit);
    has_head = offB > 0;
    first_full = tA + (offA > 0 ? 1 : 0);
    nfull = tB - first_full;
    nseg = (has_head ? 1 : 0) + nfull + (offA > 0 ? 1 : 0);
  } else {
    if (lb >= T) return false;
    nfull = nseg = (T - lb + G - 1) / G;                // tiles lb, lb + G, ...
  }
  return true;
}

// A load stream's position in the workgroup's segment list (seg_of: the kernel's own lambda)
struct RelayPos { int seg, it, it1, tile; };
template <class S>
__device__ __forceinline__ void relay_pos_init(RelayPos& q, S& seg_of) {
  int kind;
  q.seg = 0;
  seg_of(0, q.tile, q.it, q.it1, kind);
}
template <class S>
__device__ __forceinline__ bool relay_pos_next(RelayPos& q, int nseg, S& seg_of) {      // true: entered a new segment
  if (q.it + 1 < q.it1) { ++q.it; return false; }
  if (q.seg + 1 >= nseg) return false;
  int kind;
  ++q.seg;
  seg_of(q.seg, q.tile, q.it, q.it1, kind);
  return true;
}

// TAIL: the head of this tile, accumulators parked by workgroup lb - 1 (which computed them FIRST, see above).
// relay_p / relay_f: the accumulator sets / the flags behind them; a: the kernel's arguments (spin_limit, err: read here,
// where they are used); epoch: thread 0's.
template <class Args>
__device__ __forceinline__ void relay_load_head(const float* relay_p, int* relay_f, int lb, int epoch, const Args& a,
                                                f32x4 (&acc)[4][4], int tid) {
  if (tid == 0) {
    // Bounded (~2 s): the head was computed FIRST by its workgroup, so this does not spin in practice.  Should the
    // flag never come (a workspace that was not zero-filled once, a neighbour that faulted or was starved) the
    // launch must neither hang the GPU nor pass for correct: the wait gives up, raises the host-visible sticky
    // error word -- every later hnd_conv2d_igemm / hnd_sync_check then fails with HND_ERR_LAUNCH / HND_ERR_ASYNC --
    // and this tile's output is garbage by declaration.  Nothing is reset here (epoch flags, see above).
    int spin = 0;
    while (__hip_atomic_load(relay_f + (lb - 1), __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) != epoch) {
      if (++spin >= a.spin_limit) {
        if (a.err) __hip_atomic_store(a.err, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        break;
      }
      __builtin_amdgcn_s_sleep(8);
    }
  }
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  const f32x4* src = (const f32x4*)(relay_p + (size_t)(lb - 1) * RELAY_SET) + tid;
#pragma unroll
  for (int mi = 0; mi < 4; ++mi)
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) acc[mi][ni] = __builtin_nontemporal_load(src + (mi * 4 + ni) * RELAY_THREADS);
}

// HEAD: park the accumulators for workgroup lb + 1 and raise the flag -- unless raise_flag() says no (asked by thread 0
// after the barrier: conv_bstream.hip's test hook for the time-out)
template <class P>
__device__ __forceinline__ void relay_park_head(float* relay_p, int* relay_f, int lb, int epoch, P raise_flag,
                                                const f32x4 (&acc)[4][4], int tid) {
  f32x4* dst = (f32x4*)(relay_p + (size_t)lb * RELAY_SET) + tid;
#pragma unroll
  for (int mi = 0; mi < 4; ++mi)
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) __builtin_nontemporal_store(acc[mi][ni], dst + (mi * 4 + ni) * RELAY_THREADS);
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
  if (tid == 0 && raise_flag()) __hip_atomic_store(relay_f + lb, epoch, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
}

}  // namespace hnd
