// The MFMA row-tile ring shared by the k-means E-step (kmeans.hip), the top-k retrieval (topk.hip) and DBSCAN (dbscan.hip):
// "rows x rows^T with v_mfma_f32_32x32x2_f32", operand tiles of 128 rows x 32 k moved HBM -> LDS by the DMA path
// (buffer_load ... lds: no staging registers, no ds_writes).  Stateless: force-inlined device functions, templates, constants.
//
// LDS image of a tile: [128 rows][32 floats], swizzled (slic_rt_off).  A DMA instruction moves 16 bytes per lane to consecutive LDS
// addresses from a base it takes from M0, a wave-uniform 16-bit byte address: a ring reaches 64 KB, i.e. 4 stages of one 16 KB tile.
// Lane `tid` of the workgroup fills LDS slot tid & 7 of row (tid >> 3) + 32 i, so the swizzle is applied on the SOURCE side:
// the lane reads chunk cq = (tid & 7) ^ ((srow >> 1) & 7) of its row (SlicRtLane).  A DMA whose offset lies outside the buffer
// resource's range writes ZEROS to LDS: rows past an operand's end, k-tiles past D and ring steps past the last tile are sent (or
// fall) out of range and contribute 0 * x to the accumulators — exact no-ops, so the steady state has no branch.
//
// The register-operand ring (slic_rt_ring_prime / slic_rt_ring_ktile): one MFMA operand of a wave (32 rows x D) lives in NK * 16
// registers per lane, the other streams through ST = 4 stages.  Ring step s = (tile, kt) computes from stage s % ST.  Contract:
//  * every step issues 4 DMAs per lane.  prime issues steps 0 .. ST - 2; k-tile s issues step s + ST - 1 AFTER its barrier, into the
//    stage that step s - 1 computed from (every wave is past step s - 1 once it is through the barrier of step s);
//  * the counted wait: in front of the barrier of step s the DMAs of steps s + 1 .. s + ST - 2 may stay outstanding — vmcnt(4 (ST - 3)) —
//    so this wave's part of step s + 1 has LANDED (prime: vmcnt(4 (ST - 2)), step 0 has landed).  Other loads, stores or atomics a
//    kernel puts between the DMAs only make the wait stricter;
//  * the barrier of step s therefore publishes stage s + 1 (everybody's part of it), and the last quarter of step s already reads
//    the first fragments of step s + 1 from it: after the next barrier the MFMAs start at once.  `frag` carries them across calls;
//  * a kernel whose `between` reads LDS that another wave wrote since the previous barrier (k-means' exchange of a finished tile's
//    results) sets LGKM: the wait then adds lgkmcnt(0), because gfx950's back-off barrier does not imply that this wave's own ds_writes
//    have reached LDS;
//  * the ring runs ST - 1 steps past the last tile (all-zero DMAs).  They must land before the workgroup's LDS is handed to the next
//    one: every wave ends with slic_rt_wait<0>().
//
// The two-operand ring (both tiles by DMA; km_assign_dma, topk_partial_dma) keeps its loop in the kernel — the kernels differ in
// depth and in what a stage holds — and shares the addressing, the issue, the wait and one stage's MFMAs (slic_rt_compute_stage).
//
// Users.  km_assign_creg (kmeans.hip), topk_collect_qreg (topk.hip) and moco_ring (moco.hip) run the whole register-operand ring:
// slic_rt_ring_prime, then slic_rt_ring_ktile per k-tile with their issue and between-work as lambdas.  km_assign_dma and
// topk_partial_dma run the two-operand pieces.  db_tiles (dbscan.hip), hd_tiles (hdbscan.hip) and topk_collect_bf16 (topk_bf16.h)
// follow the same contract but keep the k-tile loop — wait, barrier, issue, between-work — in the kernel and share the step's MFMA
// block, slic_rt_ktile_mfma, besides the prologue pieces (slic_rt_load_frags, slic_rt_lane, slic_rt_offsets, slic_rt_issue,
// slic_rt_wait): handed to slic_rt_ring_ktile as lambdas, that work cost db_tiles two SGPRs in every instantiation and
// db_tiles<16, LINK> an SGPR spill at 512 VGPRs; with the loop left in place their register counts, LDS and scratch are the
// hand-written loop's.  km_assign_bf16 (kmeans_bf16.h) takes the prologue pieces and spells the MFMA block out; topk_partial_qreg
// (topk.hip) spells out both.  Calling slic_rt_ktile_mfma gives every topk_partial_qreg two more SGPRs (more SGPR spills at
// NK = 8 / 16) and km_assign_bf16<8> four more SGPR spills; topk_partial_qreg's prologue on the helpers kept its register
// counts but measured 0.15 - 0.3 % slower in the streaming search at D = 512, so the kernel stays as it was.
// The cause of the SGPRs: a force-inlined callee is optimised on its own first, so it arrives in
// the kernel with its qd loop unrolled and every frag[][] index constant, while the kernel's own loops are still rolled; the
// target's alloca-to-vector promotion, which runs right after inlining and takes arrays of up to 32 registers, then turns the
// 32-float frag[2][4] into ONE 32-register value that the tile loop carries whole.  Written in place, frag is indexed by the still
// rolled qd loop at that point, is left alone, and falls apart into eight 4-register values after unrolling.  The optimised IR
// of the two forms of topk_partial_qreg differs in nothing else (profiles/mfma_ktile_device_code_diff.txt); the three kernels
// that call the block get the same wide value and have the registers to spare.
// The k-means++ distance kernels keep their plain 2-stage loops.
#pragma once
#include "common.h"

#define SLIC_RT_BK 32                                // k columns per stage
#define SLIC_RT_TILE (128 * SLIC_RT_BK)              // floats of one 128-row operand tile (16 KB)
#define SLIC_RT_OOB 0xFFFFFF00u                      // a byte offset past every buffer resource's range
// for the lambdas a kernel hands to the ring functions: inlined with them, ahead of the optimiser, like code written in place
#define SLIC_RT_INLINE __attribute__((always_inline))

// 16-byte chunk c of row r lives at chunk c ^ ((r >> 1) & 7): the 16 lanes of a ds_read_b128 group (rows distinct mod 16, same
// chunk) hit 16 different 16-byte slots of the 256-byte bank row.
__device__ __forceinline__ int slic_rt_off(int row, int chunk) {
  return row * SLIC_RT_BK + ((chunk ^ ((row >> 1) & 7)) << 2);
}

// s_waitcnt vmcnt(N): at most N of this wave's vector-memory operations stay outstanding (an immediate: N is a template constant)
template <int N>
__device__ __forceinline__ void slic_rt_wait() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// The register operand of lane (r, h): MFMA step (kt, qd, t) multiplies by row[32 kt + 8 qd + 4 h + t].  D % 8 == 0: a chunk is
// inside the row or past it (zeros).
template <int NK>
__device__ __forceinline__ void slic_rt_load_frags(f32x4 (&fr)[NK][4], const float* row, int D, int h, bool row_valid = true) {
#pragma unroll
  for (int kt = 0; kt < NK; ++kt)
#pragma unroll
    for (int qd = 0; qd < 4; ++qd) {
      const int c = 32 * kt + 8 * qd + 4 * h;
      f32x4 z = {0.f, 0.f, 0.f, 0.f};
      fr[kt][qd] = (c < D && row_valid) ? *(const f32x4*)(row + c) : z;
    }
}

// DMA addressing of this thread inside a 128-row x 32-k stage
struct SlicRtLane {
  int srow;   // rows srow + 32 i of the tile
  int cq;     // SOURCE chunk of this lane (LDS slot = tid & 7)
  int klim;   // the lane's chunk of k-tile kt is inside D iff 32 kt < klim
  __device__ __forceinline__ bool kin(int kt) const { return kt * SLIC_RT_BK < klim; }
};
__device__ __forceinline__ SlicRtLane slic_rt_lane(int tid, int D) {
  const int srow = tid >> 3;
  const int cq = (tid & 7) ^ ((srow >> 1) & 7);
  return {srow, cq, D - cq * 4};
}
// byte offsets of the lane's NR rows at k-tile 0, for rows of row_bytes bytes; a row at or past `rows` is out of range for good
template <int NR>
__device__ __forceinline__ void slic_rt_offsets(unsigned (&off)[NR], const SlicRtLane& ln, unsigned row_bytes) {
#pragma unroll
  for (int i = 0; i < NR; ++i) off[i] = (unsigned)(ln.srow + 32 * i) * row_bytes + (unsigned)(ln.cq * 16);
}
template <int NR, typename R>
__device__ __forceinline__ void slic_rt_offsets(unsigned (&off)[NR], const SlicRtLane& ln, unsigned row_bytes, R rows) {
#pragma unroll
  for (int i = 0; i < NR; ++i)
    off[i] = (ln.srow + 32 * i) < rows ? (unsigned)(ln.srow + 32 * i) * row_bytes + (unsigned)(ln.cq * 16) : SLIC_RT_OOB;
}
// the lane's NR DMAs of k-tile kt into the tile at lds_tile: row i from byte base + off[i] + 128 kt, or from out of range (zeros)
// when `live` is false (ROWCHK: or when off[i] is SLIC_RT_OOB)
template <bool ROWCHK = false, int NR>
__device__ __forceinline__ void slic_rt_issue(__amdgpu_buffer_rsrc_t rsrc, float* lds_tile, int wave, const unsigned (&off)[NR],
                                              unsigned base, int kt, bool live) {
  const unsigned kb = (unsigned)kt * (SLIC_RT_BK * 4u);
#pragma unroll
  for (int i = 0; i < NR; ++i)
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (__attribute__((address_space(3))) void*)(lds_tile + (8 * wave + 32 * i) * SLIC_RT_BK), 16,
                                             (int)((live && (!ROWCHK || off[i] != SLIC_RT_OOB)) ? base + off[i] + kb : SLIC_RT_OOB), 0, 0, 0);
}

// Register-operand ring, prologue: issue(u) for the steps u = 0 .. ST - 2 of the first tile, wait for step 0, first fragments.
template <int ST, typename Issue>
__device__ __forceinline__ void slic_rt_ring_prime(f32x4 (&frag)[2][4], const float* lds, int r, int h, const Issue& issue) {
  static_assert(ST == 4, "the DMA's LDS base (M0) reaches 64 KB: 4 stages of 16 KB");
#pragma unroll
  for (int u = 0; u < ST - 1; ++u) issue(u);
  slic_rt_wait<4 * (ST - 2)>();                                // step 0 has landed
  __builtin_amdgcn_s_barrier();
#pragma unroll
  for (int i = 0; i < 4; ++i) frag[0][i] = *(const f32x4*)&lds[slic_rt_off(32 * i + r, h)];
}

// Register-operand ring: the MFMA block of one ring step, shared by slic_rt_ring_ktile and by the kernels that keep their own k-tile
// loop (their wait, barrier, issue and between-work stay in the kernel, in front of this call).  regop: this k-tile's sixteen operand
// registers; st: the stage the step computes from.  The next stage was published by this step's barrier: the last quarter fetches
// the next step's first fragments from it, and `frag` carries them across calls.  REG_A: the register operand is MFMA operand A
// (else B); NACC: accumulators in use (a ragged last tile has fewer; all four fragments are still fetched: the step after a tile's
// last belongs to a full tile).  BF16: a fragment is 8 bf16 values and feeds one v_mfma_f32_32x32x16_bf16 instead of four
// v_mfma_f32_32x32x2_f32.  k order inside every accumulator: qd ascending, t ascending, lane half 0 then 1.
// (The ring's base and a stage number, not two stage pointers: handed `lds + constant` the compiler indexes each stage by a float
// offset of its own instead of the loop's one lane address plus immediates, and every user's device code moves.)
template <bool REG_A, int NACC, bool BF16 = false>
__device__ __forceinline__ void slic_rt_ktile_mfma(f32x16 (&acc)[4], f32x4 (&frag)[2][4], const f32x4 (&regop)[4], const float* lds,
                                                   int st, int r, int h) {
  typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
  const float* Ts = lds + st * SLIC_RT_TILE;
  const float* Tn = lds + ((st + 1) & 3) * SLIC_RT_TILE;
  __builtin_amdgcn_s_setprio(1);
#pragma unroll
  for (int qd = 0; qd < 4; ++qd) {
    const int cur = qd & 1, nxt = cur ^ 1;
#pragma unroll
    for (int i = 0; i < 4; ++i)
      frag[nxt][i] = qd < 3 ? *(const f32x4*)&Ts[slic_rt_off(32 * i + r, 2 * (qd + 1) + h)]
                            : *(const f32x4*)&Tn[slic_rt_off(32 * i + r, h)];     // first fragments of the next step
    if constexpr (BF16) {
#pragma unroll
      for (int i = 0; i < NACC; ++i) {
        const bf16x8 f = __builtin_bit_cast(bf16x8, frag[cur][i]), g = __builtin_bit_cast(bf16x8, regop[qd]);
        acc[i] = REG_A ? __builtin_amdgcn_mfma_f32_32x32x16_bf16(g, f, acc[i], 0, 0, 0)
                       : __builtin_amdgcn_mfma_f32_32x32x16_bf16(f, g, acc[i], 0, 0, 0);
      }
    } else {
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int i = 0; i < NACC; ++i)
          acc[i] = REG_A ? __builtin_amdgcn_mfma_f32_32x32x2f32(regop[qd][t], frag[cur][i][t], acc[i], 0, 0, 0)
                         : __builtin_amdgcn_mfma_f32_32x32x2f32(frag[cur][i][t], regop[qd][t], acc[i], 0, 0, 0);
    }
    __builtin_amdgcn_sched_group_barrier(0x100, 4, 0);
    __builtin_amdgcn_sched_group_barrier(0x008, BF16 ? NACC : 4 * NACC, 0);
  }
  __builtin_amdgcn_s_setprio(0);
}

// Register-operand ring, k-tile kt of a tile (call it for kt = 0 .. NK - 1, unrolled: kt is a constant after inlining).
// issue(kn) issues ring step kn of the CURRENT tile, kn >= NK meaning step kn - NK of the next one; between(kt) is the kernel's own
// work of this k-tile, ahead of the MFMAs.  REG_A, NACC: as in slic_rt_ktile_mfma, which does the step's MFMAs.
template <int ST, bool REG_A, int NACC, bool LGKM, int NK, typename Issue, typename Between>
__device__ __forceinline__ void slic_rt_ring_ktile(int kt, f32x16 (&acc)[4], f32x4 (&frag)[2][4], const f32x4 (&regop)[NK][4],
                                                   const float* lds, int r, int h, const Issue& issue, const Between& between) {
  static_assert(NK % ST == 0, "a tile is a whole number of ring turns");
  if constexpr (LGKM) asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(4 * (ST - 3)) : "memory");
  else slic_rt_wait<4 * (ST - 3)>();                           // step s + 1 has landed (this wave's part of it)
  __builtin_amdgcn_s_barrier();                                // ... everybody's; and stage (kt + ST - 1) % ST has been read by all
  issue(kt + ST - 1);
  between(kt);
  slic_rt_ktile_mfma<REG_A, NACC>(acc, frag, regop[kt], lds, kt % ST, r, h);
}

// Two-operand ring: the MFMAs of one stage.  Bs / As: the stage's B and A operand tiles; the wave multiplies rows rowB + r of Bs
// by the TC row tiles of As that start at row rowA0.  LDS operands of group qd + 1 are read under group qd's MFMAs.
template <int TC>
__device__ __forceinline__ void slic_rt_compute_stage(f32x16 (&acc)[TC], const float* Bs, const float* As, int rowA0, int rowB, int r, int h) {
  f32x4 b[2], a[2][TC];
  b[0] = *(const f32x4*)&Bs[slic_rt_off(rowB + r, h)];
#pragma unroll
  for (int ct = 0; ct < TC; ++ct) a[0][ct] = *(const f32x4*)&As[slic_rt_off(rowA0 + 32 * ct + r, h)];
  __builtin_amdgcn_s_setprio(1);
#pragma unroll
  for (int qd = 0; qd < 4; ++qd) {
    const int cur = qd & 1, nxt = cur ^ 1;
    if (qd < 3) {
      b[nxt] = *(const f32x4*)&Bs[slic_rt_off(rowB + r, 2 * (qd + 1) + h)];
#pragma unroll
      for (int ct = 0; ct < TC; ++ct) a[nxt][ct] = *(const f32x4*)&As[slic_rt_off(rowA0 + 32 * ct + r, 2 * (qd + 1) + h)];
    }
    // k order inside every accumulator: qd ascending, t ascending, lane half 0 then 1 => k = 8 qd + 2 t + h ascending
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int ct = 0; ct < TC; ++ct)
        acc[ct] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[cur][ct][t], b[cur][t], acc[ct], 0, 0, 0);
    if (qd < 3) __builtin_amdgcn_sched_group_barrier(0x100, 1 + TC, 0);
    __builtin_amdgcn_sched_group_barrier(0x008, 4 * TC, 0);
  }
  __builtin_amdgcn_s_setprio(0);
}
