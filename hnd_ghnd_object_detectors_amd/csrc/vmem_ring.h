// Counted vector-memory primitives of the ring kernels (conv_bres.hip, conv_bstream.hip, conv_bx3.hip, conv_bxs.hip,
// conv_wgrad_ring.hip):
// loads the compiler cannot see into (inline asm), released by hand-counted `s_waitcnt vmcnt(N)`.  Every vector-memory
// operation of a wave retires in issue order through one counter, so "at most N outstanding" means everything but the N
// youngest has landed; hipcc waits `vmcnt(0)` at every loop header for the loads it CAN see, which empties a prefetch ring
// once per tile.  Each kernel's comments count its own N; tools/audit_bres_asm.py checks the register side in the
// disassembly (no instruction touches a ring register between its load and the wait that names it).
#pragma once
#include "common.h"

namespace hnd {

// 16 bytes from p + OFF bytes.  ACC: the destination lives in the accumulator half of the register file (VMEM can target
// it, an fp32 MFMA reads its A operand from it, the vector ALU reaches it through v_accvgpr_read).  conv_bx3.hip /
// conv_bxs.hip keep ALL ring slots there: with ring registers among the architectural ones hipcc sat at its limit and moved
// just-requested registers away before their wait.  conv_bres.hip / conv_bstream.hip keep every other slot there: beside
// two accumulator sets, all of the ring in either half ran that half out.
template <int OFF, bool ACC = true>
__device__ __forceinline__ void ring_load(f32x4& dst, const float* p) {
  if (ACC) asm volatile("global_load_dwordx4 %0, %1, off offset:%2" : "=a"(dst) : "v"(p), "n"(OFF));
  else asm volatile("global_load_dwordx4 %0, %1, off offset:%2" : "=v"(dst) : "v"(p), "n"(OFF));
}
// one byte (a row's ReLU-mask nibble), zero-extended, into the accumulator half
__device__ __forceinline__ void ring_load_byte(uint32_t& dst, const uint8_t* p) {
  asm volatile("global_load_ubyte %0, %1, off" : "=a"(dst) : "v"(p));
}

// The register-tied waits: `s_waitcnt vmcnt(N)` that names the registers it releases, so that no use of them moves above
// it.  The tied wait of a slot must be ONE statement on every path: tied waits in the two arms of a branch made hipcc merge
// the ring registers with copies placed BEFORE the wait in one arm.  One overload per arity in use -- two, three or four ring
// registers (ACC as above), four + one or two architectural ones (the B-streamed kernel's parked B loads), eight
// accumulator-half ones.
template <int N, bool ACC>
__device__ __forceinline__ void ring_wait(f32x4& a0, f32x4& a1) {
  if (ACC) asm volatile("s_waitcnt vmcnt(%2)" : "+a"(a0), "+a"(a1) : "n"(N));
  else asm volatile("s_waitcnt vmcnt(%2)" : "+v"(a0), "+v"(a1) : "n"(N));
}
template <int N, bool ACC>
__device__ __forceinline__ void ring_wait(f32x4& a0, f32x4& a1, f32x4& a2) {
  if (ACC) asm volatile("s_waitcnt vmcnt(%3)" : "+a"(a0), "+a"(a1), "+a"(a2) : "n"(N));
  else asm volatile("s_waitcnt vmcnt(%3)" : "+v"(a0), "+v"(a1), "+v"(a2) : "n"(N));
}
template <int N, bool ACC>
__device__ __forceinline__ void ring_wait(f32x4& a0, f32x4& a1, f32x4& a2, f32x4& a3) {
  if (ACC) asm volatile("s_waitcnt vmcnt(%4)" : "+a"(a0), "+a"(a1), "+a"(a2), "+a"(a3) : "n"(N));
  else asm volatile("s_waitcnt vmcnt(%4)" : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3) : "n"(N));
}
template <int N, bool ACC>
__device__ __forceinline__ void ring_wait(f32x4& a0, f32x4& a1, f32x4& a2, f32x4& a3, f32x4& b0) {
  if (ACC) asm volatile("s_waitcnt vmcnt(%5)" : "+a"(a0), "+a"(a1), "+a"(a2), "+a"(a3), "+v"(b0) : "n"(N));
  else asm volatile("s_waitcnt vmcnt(%5)" : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(b0) : "n"(N));
}
template <int N, bool ACC>
__device__ __forceinline__ void ring_wait(f32x4& a0, f32x4& a1, f32x4& a2, f32x4& a3, f32x4& b0, f32x4& b1) {
  if (ACC)
    asm volatile("s_waitcnt vmcnt(%6)" : "+a"(a0), "+a"(a1), "+a"(a2), "+a"(a3), "+v"(b0), "+v"(b1) : "n"(N));
  else
    asm volatile("s_waitcnt vmcnt(%6)" : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(b0), "+v"(b1) : "n"(N));
}
template <int N, class T>      // T = f32x4 (ring slots, residual rows) or uint32_t (mask bytes)
__device__ __forceinline__ void ring_wait(T& a0, T& a1, T& a2, T& a3, T& a4, T& a5, T& a6, T& a7) {
  asm volatile("s_waitcnt vmcnt(%8)"
               : "+a"(a0), "+a"(a1), "+a"(a2), "+a"(a3), "+a"(a4), "+a"(a5), "+a"(a6), "+a"(a7)
               : "n"(N));
}

// LDS-DMA: 64 lanes x 16 bytes from per-lane global addresses to lds_dst + 16 * lane (M0 is compiler-reserved: saved,
// written and restored inside the one statement)
__device__ __forceinline__ void glds16(const void* gsrc, unsigned lds_dst) {
  unsigned keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
               : "=&s"(keep)
               : "v"(gsrc), "s"(lds_dst)
               : "memory");
}

}  // namespace hnd
