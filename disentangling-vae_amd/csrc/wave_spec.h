// Wave-specialisation primitives: the LDS-DMA transfer, the counted waits and the bare barrier of every kernel here that
// keeps loader waves next to compute waves (conv_down_dma.hip, conv_thin_ws.hip, gemm_dma.hip, fc_chain.hip, conv4_end.h,
// conv_mfma_common.h, conv_up_thin_mm.hip).  The ONE home of s_waitcnt / s_barrier / global_load_lds in csrc/.
//
// The rules these exist to enforce (a mistake in any of them does not fault: it gives wrong values on some waves of some
// launches):
//   1. M0 is written in the statement that reads it.  global_load_lds_dwordx4 takes its LDS base from M0; the compiler
//      reserves M0 for itself and preserves nothing in it between two statements, so `s_mov_b32 m0` and the transfer are
//      one asm string (lds_dma16, lds_dma16_masked), or the compiler writes M0 itself (lds_dma16_tracked).
//   2. A transfer issued from inline asm is invisible to the compiler's wait bookkeeping: no s_waitcnt is emitted for it
//      and __syncthreads() does not wait for it.  Its data is retired by hand, in this order: a counted wait in the wave
//      that issued it (wait_vmcnt<N>: vector-memory operations complete in issue order, loads and stores in one counter,
//      so "all but the N newest" names exactly the tile that must have landed), THEN a workgroup barrier, THEN the ds_read
//      of the consumer.  The transfer has no destination register, so nothing else can go wrong with it.
//   3. That barrier is barrier_nofence(), never __syncthreads(): in front of a __syncthreads() the compiler drains vmcnt
//      to 0, which would retire the very transfers the loaders keep in flight across the barrier (the next tiles of the
//      ring).  The bare s_barrier orders nothing by itself; the orderings that matter come from the waits of rule 2 on
//      the loader side and from wait_lgkmcnt0() ("my LDS reads / writes have returned") or the data dependence
//      MFMA <- ds_read on the compute side.
//
// Two kinds of transfer, both kept: the asm forms are NOT counted by the compiler (a wave that also computes keeps them in
// flight under its own LDS reads); lds_dma16_tracked IS counted (the compiler puts a vmcnt(0) in front of the wave's next
// LDS read: fine for a wave that only loads, fatal for one that also multiplies).  A call site is one kind on purpose.
//
// M0 note: the asm forms name "m0" as a clobber instead of saving and restoring it around the statement.  The compiler
// answers with -Winline-asm ("clobber list contains reserved registers"; silenced below) and does not promise to honour
// the clobber.  What goes through M0 in these kernels is the LDS base of lds_dma16_tracked, which the compiler writes
// right in front of each transfer; fc_chain.hip is the one file that mixes both kinds in one kernel.  Saving M0 in the
// statement would change the machine code of every loader loop and is left to a change of its own.
#pragma once

namespace dvae {

#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winline-asm"     // "m0" in the clobber lists: see the note above

// one LDS-DMA transfer: lane l of the wave moves 16 bytes from its own global address to LDS byte lds_addr + 16 l
// (lds_addr wave-uniform; 1 KB per wave instruction, the LDS side is lane-linear)
__device__ __forceinline__ void lds_dma16(const void* gsrc, unsigned lds_addr) {
  asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, off" ::"v"(gsrc), "s"(lds_addr) : "memory", "m0");
}

// the same from a wave-uniform base + a 32-bit offset per lane, for the lanes of `lanes` only: every ACTIVE lane l moves 16
// bytes to LDS byte lds_addr + 16 l, inactive lanes leave their LDS bytes alone.  Called with all 64 lanes active: the lane
// mask is applied to EXEC around the instruction and EXEC is set back to all ones.
__device__ __forceinline__ void lds_dma16_masked(const void* sbase, unsigned voff, unsigned lds_addr, unsigned long long lanes) {
  asm volatile("s_mov_b32 m0, %2\n\ts_mov_b64 exec, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1\n\ts_mov_b64 exec, -1" ::"v"(voff),
               "s"(sbase), "s"(lds_addr), "s"(lanes)
               : "memory", "m0");
}

#pragma clang diagnostic pop

// the compiler-tracked transfer: same instruction, issued through the builtin, so the compiler writes M0 and COUNTS it in
// its own waits (the asm forms above are not counted).  lds_ptr wave-uniform.
__device__ __forceinline__ void lds_dma16_tracked(const void* gptr, void* lds_ptr) {
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)gptr, (__attribute__((address_space(3))) void*)lds_ptr,
                                   16, 0, 0);
}

// all but the N newest vector-memory operations of this wave have completed
template <int N>
__device__ __forceinline__ void wait_vmcnt() {
  static_assert(N >= 0 && N < 64, "vmcnt is a 6-bit field");
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// every LDS (and scalar-memory) operation of this wave has returned.  The s_waitcnt immediate of gfx9: vmcnt in bits
// 3:0 and 15:14, expcnt in 6:4, lgkmcnt in 11:8 -- 0xC07F = vmcnt 63 and expcnt 7 (no wait), lgkmcnt 0.
__device__ __forceinline__ void wait_lgkmcnt0() { __builtin_amdgcn_s_waitcnt(0xC07F); }

// workgroup barrier WITHOUT the compiler's vmcnt(0) drain (rule 3)
__device__ __forceinline__ void barrier_nofence() { asm volatile("s_barrier" ::: "memory"); }

}  // namespace dvae
