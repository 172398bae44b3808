// Wave-level inline-asm primitives of the hand-scheduled MFMA kernels (gemm2.hip, conv_gemm.hip, conv_stream.hip, conv_block.hip,
// conv_row64.hip, conv_s2.hip, linkage.hip): hidden stores, LDS-DMA pieces, uniform pointers, counted waits, the pixel swizzle.
// One definition each, with what was measured about it.  Asm statements that exist in one kernel only (gemm2_kernel's eight-piece
// DMA, conv_stream's six-piece DMA and hidden load, linkage's sc1 exchange, the empty register-pinning statements) live in that
// kernel's file.  The bf16 MFMA on two uint4 is Mma16<bf16_t>::run (common.h).
//
// Why any of this is inline asm: hipcc's waitcnt pass keeps one in-order count (vmcnt) for loads, LDS-DMA pieces and stores.  It
// drains vmcnt(0) in front of every ds_read that follows an LDS-DMA issue, and any wait it places for a load result also waits
// for every store issued before that load.  What it does not see it does not wait for: the kernels that use these primitives
// count vmcnt themselves (wait_vm<N>), and say at each wait what it covers.
#pragma once
#include "common.h"

namespace rvb {

// unsigned vectors as "v" operands of asm statements (uint4 / uint2 are structs: not accepted there)
typedef unsigned u32x4_t __attribute__((ext_vector_type(4)));
typedef unsigned u32x2_t __attribute__((ext_vector_type(2)));

// One 16-byte global store the compiler's waitcnt bookkeeping does not see.  It would otherwise wait for a store before the next
// pass touches the registers the store read, i.e. drain the stores one by one, and every wait it places for a later load also
// waits for the stores in front of it (gemm2p_kernel's full-tile epilogue has the figures).  Sound next to the compiler's own
// counting of loads: hidden stores are OLDER than the loads it waits for, so they only make such a wait cover more than it thinks.
// s_nop 1: gfx950 wants TWO wait states between a store of more than 8 bytes and a VALU write of its data registers -- hipcc
// places them for the stores it knows (one unrelated VALU instruction + s_nop 0 in its own code), its hazard recognizer does
// not look into inline asm, and with one (s_nop 0) 0.11 % of the stored words carried the NEXT value of the register on a
// busy chip (scripts/micro/store_hazard.hip, profiles/archive/r04_store_hazard.txt; in the first form of gemm2p's epilogue: 16-128
// wrong elements per million in one kernel whose register allocation put a v_add / v_mad right behind a store).  An LDS
// read into the same registers right behind the store is safe (0 of 2.7e8 words).
__device__ inline void store16_hidden(void* q, unsigned a, unsigned b, unsigned c, unsigned d) {
  const u32x4_t v = {a, b, c, d};
  asm volatile("global_store_dwordx4 %0, %1, off\n\ts_nop 1" ::"v"(q), "v"(v) : "memory");
}
__device__ inline void store16_hidden(void* q, const uint4& v) { store16_hidden(q, v.x, v.y, v.z, v.w); }
// ... and its 8-byte sibling (gemm2p's ACT_GLU: a lane's eight columns are four gated values)
__device__ inline void store8_hidden(void* q, unsigned a, unsigned b) {
  const u32x2_t v = {a, b};
  asm volatile("global_store_dwordx2 %0, %1, off\n\ts_nop 1" ::"v"(q), "v"(v) : "memory");
}

// LDS-DMA (`global_load_lds_dwordx4`: HBM -> LDS, no VGPR round trip, no ds_write pass).  One instruction writes a 1-KiB piece:
// 64 lanes x 16 bytes in lane order, at the wave-uniform LDS address M0 carries.  Inline asm on purpose: the waitcnt pass does
// not see the pieces (it would otherwise drain vmcnt(0) before every ds_read that follows a DMA issue), so the explicit counted
// wait of the kernel's loop is what orders them.  M0 belongs to the compiler: saved and restored.
//
// one piece from a per-lane global pointer
__device__ inline void lds_dma1(const void* g, unsigned lds) {
  unsigned keep;
  asm volatile(
      "s_mov_b32 %0, m0\n\t"
      "s_mov_b32 m0, %2\n\t"
      "s_nop 0\n\t"
      "global_load_lds_dwordx4 %1, off\n\t"
      "s_mov_b32 m0, %0"
      : "=&s"(keep)
      : "v"(g), "s"(lds)
      : "memory");
}
// one piece from a scalar base (uniform_ptr) + per-lane 32-bit byte offsets
__device__ inline void lds_dma1(unsigned off, const void* sbase, unsigned lds) {
  unsigned keep;
  asm volatile(
      "s_mov_b32 %0, m0\n\t"
      "s_mov_b32 m0, %3\n\t"
      "s_nop 0\n\t"
      "global_load_lds_dwordx4 %1, %2\n\t"
      "s_mov_b32 m0, %0"
      : "=&s"(keep)
      : "v"(off), "s"(sbase), "s"(lds)
      : "memory");
}
// two pieces, consecutive in LDS (0x400 apart), from a scalar base + per-lane offsets
__device__ inline void lds_dma2(unsigned off0, unsigned off1, const void* sbase, unsigned lds) {
  unsigned keep;
  asm volatile(
      "s_mov_b32 %0, m0\n\t"
      "s_mov_b32 m0, %4\n\t"
      "s_nop 0\n\t"
      "global_load_lds_dwordx4 %1, %3\n\t"
      "s_add_u32 m0, m0, 0x400\n\t"
      "s_nop 0\n\t"
      "global_load_lds_dwordx4 %2, %3\n\t"
      "s_mov_b32 m0, %0"
      : "=&s"(keep)
      : "v"(off0), "v"(off1), "s"(sbase), "s"(lds)
      : "memory", "scc");
}
// a wave-uniform pointer, provably so for the "s" operand of an LDS-DMA (uniform values that went through a VALU division live
// in VGPRs otherwise); folds away when the value already sits in SGPRs
__device__ inline const char* uniform_ptr(const char* q) {
  const unsigned long long v = (unsigned long long)q;
  const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v), hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
  return (const char*)(((unsigned long long)hi << 32) | lo);
}

// Counted waits.  vmcnt is one in-order queue of this wave's loads, LDS-DMA pieces and stores: wait_vm<N> returns when all but the
// youngest N have completed (a store: acknowledged by the L2).
template <int N> __device__ inline void wait_vm() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }
// ... and every LDS access of this wave has returned (in front of a barrier behind which its buffer is requested or written again)
template <int N> __device__ inline void wait_vm_lds() { asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(N) : "memory"); }
__device__ inline void wait_lds() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }

// byte offset of (pixel g, 16-byte chunk c) in a [pixel][64 B] image whose chunks are XOR-swizzled with bit 2 of the pixel index
// (chunk ^= 2 for pixels 4-7 mod 8; on the source side of the LDS-DMA, on the write side of a ds_write): the plain layout serves a
// ds_read_b128 of 16 consecutive pixels with a 2-way bank conflict in every lane group, this one covers all 64 banks once
// (conv_block.hip has the counters)
__device__ inline unsigned pixel_swz(unsigned g, unsigned c) { return g * 64u + ((c ^ (((g >> 2) & 1u) << 1)) << 4); }

}  // namespace rvb
