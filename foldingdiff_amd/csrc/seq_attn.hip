// BertSelfAttention of a whole sequence in ONE kernel: the q | k | v projection (HF 4.11.3 BertSelfAttention.query / key / value,
// constructed at foldingdiff/modelling.py:271, called :473-480) AND the attention with the relative_key term, the additive -10000
// key mask and the softmax -- q, k and v never reach HBM (the two-kernel path writes 302 MB of them per layer at BASELINE C2 and
// reads them back: 37 % of a step's stored bytes).
//
// Arithmetic: the same fp16 hi / lo split triples on v_mfma_f32_32x32x16_f16, in the same order per accumulator, as gemm_img.hip
// (projection) and attention_img.hip (S^T = K Q^T, the band R^T = E Q^T, O^T = V^T P^T); the ctx image this kernel writes is
// BIT-IDENTICAL to the one the two kernels write (tests/test_gpu_parity.py).
//
// Structure.  One 4-wave workgroup (one wave per SIMD, 512 registers each) per CU, persistent over sequences of <= 128 rows:
//  * wave w owns token rows 32 w .. 32 w + 31 of the sequence; its rows of the hidden state (K = 384: 12 k-tiles x 2 k16 steps x
//    (hi, lo) x 4 registers = 192 registers) are loaded ONCE per sequence and stay in registers as MFMA operands (B operand of the
//    swapped form D^T = W h^T for q and k: a lane owns a token; A operand of the normal form for v: a lane owns a feature, which is
//    what O^T = V^T P^T wants);
//  * the weights stream head by head through an LDS ring: a stage = one k-tile of a head's 96 rows (q_h | k_h | v_h), 12 KiB,
//    unit-major ([unit][96 rows][16 B]: conflict-free 16-byte fragment reads), copied by LDS-DMA three pieces per wave, ring of 4,
//    ONE workgroup barrier per stage;
//  * per head the epilogue turns the three 32 x 32 accumulators into: q_h -> this wave's B operand registers (bias, scale, hi / lo
//    split, one half-wave exchange); k_h -> LDS in the attention kernel's unit-major piece layout; v_h -> LDS as V^T blocks;
//  * the attention of head h-1 is SOFTWARE PIPELINED into the twelve stages of head h's projection (slots, see attn_slot): with
//    one wave per SIMD there is no partner wave to hide a dependent chain behind (S^T -> band -> softmax -> P V -> store), so every
//    link of that chain sits one stage (1100-2000 cycles) behind the previous one and the softmax / skew arithmetic sits between
//    the projection's matrix instructions (plain fp32 VALU: this file is compiled with -fno-slp-vectorize).  The workgroup's
//    (sequence, head) items form ONE stream: iteration i projects item i and runs the attention of item i - 1, across sequence
//    boundaries too (the next sequence's hidden state replaces the current one in place, k-tile by k-tile, during the last head);
//    only the first item's projection and the last item's attention -- once per launch -- are code of their own.
//  * what bounds it (profiles/r05_seq_attn_notes.log): every stage fits T = 32 cycles x MFMAs + ~4 cycles x (VALU + LDS
//    instructions) -- a wave's own vector work does not overlap its own matrix instructions; 294 MFMAs + ~1850 other instructions per
//    item = 18.5 k cycles, 45 % of the matrix pipe.
// Wave-uniform branches inside the fused iteration would split the stage into separately scheduled blocks, so every wave always
// computes all 128 query / key rows: rows beyond the sequence's rows are finite garbage whose keys get -inf scores (probability
// exactly 0) and whose ctx stores fall outside the buffer descriptor (dropped by the hardware).
#include <cstdlib>
#include <type_traits>

#include "fdmi_kernels.h"
#include "img_common.h"
#include "launch_common.h"

#ifndef FDMI_SA_SCHED
#define FDMI_SA_SCHED 0  // 0: the source order of the slots is the schedule (sched_barrier between them); 1: the slots' order only holds for
                         // the MFMAs, everything else of a stage is dealt out evenly behind them with sched_group_barrier
#endif
#ifndef FDMI_SA_SKIP
#define FDMI_SA_SKIP 0  // ablation builds (wrong results, and a skipped epilogue lets hipcc drop the projection it feeds): bit s = the
                        // attention slice of stage s is left out
#endif
#ifndef FDMI_SA_EDGES
#define FDMI_SA_EDGES 1  // 1: the first item's projection and the last item's attention run alone (their own code); 0: one loop body
                         // for everything -- iteration 0 runs an attention on garbage, the last one a projection for nothing
#endif
#ifndef FDMI_SA_SUBSTAGE
#define FDMI_SA_SUBSTAGE 0  // instrumented build (FDMI_STAMPS=1): the stage whose pieces get stamps of their own
#endif
#ifndef FDMI_SA_DBG
#define FDMI_SA_DBG 0  // ablation builds (wrong results): 1 = no attention slices, 2 = no projection MFMAs, 4 = no ctx stores
#endif

namespace fdmi {
namespace sa {

template <int V> using IC = std::integral_constant<int, V>;
template <int LO, int HI, class F>
__device__ __forceinline__ void static_for(F&& f) {
  if constexpr (LO < HI) {
    f(IC<LO>{});
    static_for<LO + 1, HI>(f);
  }
}

typedef const __attribute__((address_space(3))) float* lds_cf32_t;
typedef const __attribute__((address_space(3))) u32x4* lds_cu128_t;
__device__ __forceinline__ unsigned lds_addr(const void* p) { return (unsigned)(unsigned long long)(lds_ptr_t)(const_cast<void*>(p)); }
__device__ __forceinline__ float lds_f32(unsigned a) { return *(lds_cf32_t)(unsigned long long)a; }
__device__ __forceinline__ u32x4 lds_u128(unsigned a) { return *(lds_cu128_t)(unsigned long long)a; }

constexpr float PS = 1024.0f;  // probabilities are <= 1
constexpr float kLog2e = 1.44269504088896341f;
constexpr float kInvSqrtD = 0.17677669529663687f;  // 1 / sqrt(32)

__device__ __forceinline__ float exp2_neg(float x) { return __builtin_amdgcn_exp2f(x); }
__device__ __forceinline__ void pair_halves(float x, float& lo, float& hi) {  // (attention_img.hip)
  unsigned a = __builtin_bit_cast(unsigned, x), b = a;
  swap32(a, b);
  lo = __builtin_bit_cast(float, a);
  hi = __builtin_bit_cast(float, b);
}
__device__ __forceinline__ float pair_max(float x) {
  float lo, hi;
  pair_halves(x, lo, hi);
  return fmaxf(lo, hi);
}
__device__ __forceinline__ float pair_sum(float x) {
  float lo, hi;
  pair_halves(x, lo, hi);
  return lo + hi;
}

// One int of a small device table as a SCALAR load, complete on return.  Inside the item loop hipcc reads such tables with
// global_load_dword (the kernel also stores, so the tables are not provably invariant), and the vmcnt(0) it then puts in front of the
// first use drains the weight stream.
__device__ __forceinline__ int sload(const int* base, int index) {
  int v;
  asm volatile("s_load_dword %0, %1, %2\n\ts_waitcnt lgkmcnt(0)" : "=s"(v) : "s"(base), "s"(index * 4) : "memory");
  return v;
}

// three of them in flight together (a sequence's row range, row count and length: one after the other they cost ~1100 ticks each
// on their first, cold, use: profiles/r05_seq_attn_notes.log)
__device__ __forceinline__ void sload3(const int* a, int ia, const int* b, int ib, const int* c, int ic, int& x, int& y, int& z) {
  asm volatile("s_load_dword %0, %3, %4\n\ts_load_dword %1, %5, %6\n\ts_load_dword %2, %7, %8\n\ts_waitcnt lgkmcnt(0)"
               : "=&s"(x), "=&s"(y), "=&s"(z)
               : "s"(a), "s"(ia * 4), "s"(b), "s"(ib * 4), "s"(c), "s"(ic * 4)
               : "memory");
}

#ifndef FDMI_SA_ASM_MFMA
#define FDMI_SA_ASM_MFMA 1  // 1: the attention's MFMAs are written in assembly with their accumulators in VGPRs
#endif
// The attention's accumulators (S^T, the band tiles, O^T) are VALU / LDS operands right after their last MFMA.  hipcc gives the
// builtin's result the AGPR half of the register file and copies it out (16 v_accvgpr_read per tile, ~160 per head, in a kernel
// that is bound by its instruction count); written in assembly the accumulator IS a VGPR tuple.  The compiler cannot see that these
// statements are matrix instructions, so the hazards are this file's business: their A / B operands come from LDS reads (the
// compiler still waits for those) or were written by VALU instructions several MFMAs earlier; their results are read by other
// instructions no sooner than two projection MFMAs (64 cycles) later; chained MFMAs name exactly the same accumulator tuple.
__device__ __forceinline__ void mfma_acc(f32x16& d, const f16x8& a, const f16x8& b) {  // d += a b
#if FDMI_SA_ASM_MFMA
  asm volatile("v_mfma_f32_32x32x16_f16 %0, %1, %2, %0" : "+v"(d) : "v"(a), "v"(b));
#else
  d = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, d, 0, 0, 0);
#endif
}
__device__ __forceinline__ void mfma_new(f32x16& d, const f16x8& a, const f16x8& b) {  // d = a b
#if FDMI_SA_ASM_MFMA
  asm volatile("v_mfma_f32_32x32x16_f16 %0, %1, %2, 0" : "=&v"(d) : "v"(a), "v"(b));
#else
  const f32x16 z = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  d = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, z, 0, 0, 0);
#endif
}

constexpr int T = 4, LP = 128;          // key tiles of 32, keys per sequence tile
constexpr int NST = 4;                  // weight ring stages
constexpr int KT_BYTES = 96 * 128;      // one k-tile of a head's 96 weight rows
constexpr int OFF_E = 0;                // distance table image, 256 rows x 128 B
constexpr int OFF_K = 32768;            // K of the current head: 128 keys x 128 B, unit-major pieces
constexpr int OFF_V = OFF_K + 16384;    // V^T of the current head: 4 key blocks x 32 d x 128 B
constexpr int OFF_R = OFF_V + 16384;    // skew scratch: 4 waves x two 4 KiB tile slots
constexpr int OFF_W = OFF_R + 32768;    // weight ring
constexpr int OFF_B = OFF_W + NST * KT_BYTES;  // bias q | k | v at the images' scales, 3 x 384 floats
constexpr int SMEM = OFF_B + 3 * 384 * 4;      // 152,064 B

// The relative_key band as operations on band tiles (attention_img.hip: band_op): M(q) R^T tile q = E_q Q^T into accumulator q & 1,
// W(q) accumulator -> scratch slot q & 1, G(q) S^T tile T-1-q += band values of the tile pair (q, q+1).  Program order
//     M0 M1 W0 W1 | M2 G0 W2 | M3 G1 W3 | M4 G2 W4 | G3        (one group per attention slice)

template <int NKT, bool PROF>
__global__ __launch_bounds__(256) void seq_attn_kernel(SeqAttnArgs p) {
  static_assert(NKT == 12 || NKT == 6, "d_model 384 or 192");
  constexpr int H = NKT;              // heads of size 32
  constexpr int SPS = 12 / NKT;       // attention slices per projection stage
  constexpr int D = 32 * NKT;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wq = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int half = lane >> 5, l31 = lane & 31;
  unsigned char* Es = smem + OFF_E;
  float* par = reinterpret_cast<float*>(smem + OFF_B);
  // the LDS address of `smem` as an opaque scalar: every LDS address below is this + a constant + lane arithmetic.  Formed from the
  // generic pointer at its point of use, an address costs the pointer cast's null check (seven scalar instructions), and hipcc
  // re-forms addresses inside the item loop rather than keep them in registers
  unsigned smem0 = __builtin_amdgcn_readfirstlane(lds_addr(smem));
  asm volatile("" : "+s"(smem0));
  const unsigned a_Es = smem0 + OFF_E, a_Ks = smem0 + OFF_K, a_Vt = smem0 + OFF_V, a_Rw = smem0 + OFF_R + (unsigned)(wq * 8192),
                 a_Wr = smem0 + OFF_W, a_par = smem0 + OFF_B;
  const unsigned rw_lds = a_Rw;

  // ---- once per workgroup: bias at the scale of the image its column feeds ((acc os + b) sc == fma(acc, os sc, b sc) exactly for the
  // power-of-two sc: gemm_img.hip), the distance table (attention_img.hip, ELDS: LDS row rho holds table row clamp(rho - esh))
  for (int i = tid; i < 3 * D; i += 256) {
    const float sc = i < D ? p.q_scale : (i < 2 * D ? p.k_scale : p.v_scale);
    par[i] = p.bias[i] * sc;
  }
  const int esh = LP > p.maxpos ? LP - p.maxpos : 0;
  {
    const int nrow_e = 2 * p.maxpos - 1;
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<unsigned char*>(reinterpret_cast<const unsigned char*>(p.demb)), 0, nrow_e * 128, 0x00020000);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int piece = wq + 4 * i;  // LDS rows 8 piece .. 8 piece + 7
      const int rho = 8 * piece + (lane >> 3);
      int row = rho - esh;
      row = row < 0 ? 0 : (row > nrow_e - 1 ? nrow_e - 1 : row);
      dma16(rs, (lds_ptr_t)(Es) + piece * 1024, row * 128 + (((lane & 7) ^ ((rho >> 1) & 7)) << 4), 0);
    }
  }
  // band geometry of this lane (attention_img.hip): MFMA row i of a band tile computes band row pi(i)
  const int pi31 = (l31 & 24) | ((l31 & 3) << 1) | ((l31 >> 2) & 1);
  // gather addresses (attention_img.hip): query l31, key kl = kl_r + 4 half needs band index j = l31 - kl + 31 of its tile pair, byte
  // j * 128 + 4 l31 of the pair's 63 consecutive band rows.  Even pairs have their lower tile in slot 0: address gb + (27 - kl_r) * 128,
  // an immediate offset.  Odd pairs have the slots swapped (lower tile in slot 1): the same address + 4096, wrapped around the wave's
  // 8 KiB scratch (which is 8 KiB aligned) -- one add and one and-or per score instead of a sixteen-register address table, which
  // this kernel cannot afford (attention_img.hip keeps the table).
  const unsigned gb = a_Rw + (unsigned)((l31 - 4 * half + 4) * 128 + 4 * l31);
  const unsigned gwrap = (unsigned)((l31 - 4 * half + 4) * 128 + 4 * l31) + 4096u;  // offset inside the scratch, before wrapping
  const unsigned rw_base = a_Rw;
  static_assert(OFF_R % 8192 == 0, "the skew scratch of a wave must be 8 KiB aligned");
  // band tile operand rows (attention_img.hip, ELDS): MFMA row l31 -> band row pi31 of the tile; unit u of LDS row rp sits at position
  // u ^ ((rp >> 1) & 7).  The lane's four units 2 k + half, k = 0..3, differ from unit `half` in bits 1-2 only, and the XOR commutes:
  // address of unit 2 k + half = eaddr0 ^ (32 k) -- one register instead of four
  unsigned eaddr0;
  {
    const int rp = p.maxpos - LP + esh + 32 * wq + pi31;
    eaddr0 = a_Es + (unsigned)(rp * 128 + ((half ^ ((rp >> 1) & 7)) << 4));
    asm volatile("" : "+v"(eaddr0));
  }
  // K / V addresses of this lane: key (row) 32 wq + l31 of the head's K tile, feature row l31 of the V^T blocks
  const int ksz = (l31 >> 3) & 1;
  // the lane's units 2 c + 4 plane + half sit at positions (2 c + 4 plane + half) ^ ksz = 2 c + 4 plane + (half ^ ksz): the lane part
  // is folded into the base, the rest is an immediate offset
  const unsigned k_rd = a_Ks + (unsigned)((l31 >> 3) * 1024 + (l31 & 7) * 16 + ((half ^ ksz) << 7));  // + 4096 t + (2 c + 4 plane) * 128
  const unsigned k_wr = k_rd + (unsigned)(wq * 4096);
  const int vsz = vt_swz(l31);
  const unsigned v_rd = a_Vt + (unsigned)(l31 * 128);  // + 4096 t + ((unit ^ vsz) << 3)
  const unsigned v_wr = v_rd + (unsigned)(wq * 4096);
  const unsigned par_base = a_par;
  const unsigned w_rd = a_Wr + (unsigned)(l31 * 16 + half * 1536);  // + slot * KT_BYTES + (2 c + 4 plane) * 1536 + 512 j

  const float s_scale = kLog2e * kInvSqrtD / (p.q_scale * p.k_scale);  // raw MFMA sums -> log2 domain
  const float mask_raw = -10000.0f * kLog2e / s_scale;                  // (1 - mask) * -10000 at the raw scale (modelling.py:452)
  const float oss_q = p.acc_scale * p.q_scale, oss_k = p.acc_scale * p.k_scale, oss_v = p.acc_scale * p.v_scale;
  const f32x16 zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};

  // ---- the weight stream: positions (sequence, head, k-tile) of this workgroup, one 12 KiB stage each; the stream does not stop at
  // a sequence's end (the next sequence's first stages are requested during the last head)
  const int nseq = (p.B - (int)blockIdx.x + (int)gridDim.x - 1) / (int)gridDim.x;
  int pos = 0;     // position being computed
  int w_src = 0;   // byte offset of the next position to request inside the weight image: (head, k-tile) wraps after the last head
  int w_slot = 0;  // byte offset of the ring slot it goes to
  const __amdgpu_buffer_rsrc_t rs_w =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned char*>(p.wimg), 0, H * NKT * KT_BYTES, 0x00020000);
  // (the stream simply runs on past the workgroup's last position: what it requests there lands in free slots and is never read)
  // WRAP: the position requested is k-tile 0 of a head (stage NKT - 3 of an item requests it): only there can the stream have
  // reached the end of the weight image
  auto issue_w = [&](auto WRAP) __attribute__((always_inline)) {
    if constexpr (decltype(WRAP)::value) w_src = w_src == H * NKT * KT_BYTES ? 0 : w_src;
    const lds_ptr_t dst = (lds_ptr_t)(unsigned long long)(a_Wr + (unsigned)__builtin_amdgcn_readfirstlane(w_slot));
    const int so = __builtin_amdgcn_readfirstlane(w_src);
#pragma unroll
    for (int k = 0; k < 3; ++k) dma16(rs_w, dst + (wq + 4 * k) * 1024, lane * 16, so + (wq + 4 * k) * 1024);
    w_src += KT_BYTES;
    w_slot = w_slot + KT_BYTES == NST * KT_BYTES ? 0 : w_slot + KT_BYTES;
  };

  // ---- per-sequence state
  f16x8 hh[NKT][2], hl[NKT][2];  // the wave's rows of the hidden state
  f32x16 acc[3];                 // q_h | k_h (swapped form) | v_h (normal form) of the head being projected
  f16x8 qh[2], ql[2];            // Q operand of the head whose attention is running
  f32x16 sacc[T], racc[2], oacc;
  float mt = 0.f, nm = 0.f, l_run = 1.f;
  // the sequence of the head whose ATTENTION is running (one item behind the projection; nrows 0: every ctx store is dropped)
  int row0 = 0, nrows = 0, Lb = LP, len = LP;

  const __amdgpu_buffer_rsrc_t rs_h = __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned char*>(p.himg), 0, p.himg_bytes, 0x00020000);
  // the lane's rows of k-tile kt of the hidden state of the sequence whose first row is r0 (rows beyond the image read as zeros)
  auto load_h_kt = [&](auto KT, int r0) __attribute__((always_inline)) {
    constexpr int kt = decltype(KT)::value;
    int ln;  // (an opaque copy of the lane index: nothing derived from it lives across the loop, see ctx_store)
    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(ln));
    const int row = r0 + 32 * wq + (ln & 31);
    const unsigned hoff = (unsigned)(((row >> 5) * (NKT * 256) + (row & 31)) * 16 + (ln >> 5) * 512);
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      hh[kt][c] = __builtin_bit_cast(f16x8, __builtin_amdgcn_raw_buffer_load_b128(rs_h, (int)hoff, (kt * 8 + 2 * c) * 512, 0));
      hl[kt][c] = __builtin_bit_cast(f16x8, __builtin_amdgcn_raw_buffer_load_b128(rs_h, (int)hoff, (kt * 8 + 4 + 2 * c) * 512, 0));
    }
  };

  const bool rec = PROF && blockIdx.x == 0 && p.stamps != nullptr;
  unsigned long long* st = PROF ? p.stamps + (size_t)wq * 64 * 16 : nullptr;
  int slot = 0;
#define FD_STAMP(i) do { if (PROF) { if (rec && slot < 64 && lane == 0) st[slot * 16 + (i)] = __builtin_amdgcn_s_memtime(); } } while (0)
#define FD_SB() __builtin_amdgcn_sched_barrier(0)
#ifndef FDMI_SA_DUMP
#define FDMI_SA_DUMP 0  // debug build: wave 0 of workgroup 0 dumps registers of the attention that runs in iteration FDMI_SA_DUMP (needs FDMI_STAMPS=1)
#endif
  // register dump: out[(base + i) * 64 + lane] = value i of this lane
  auto dump16 = [&](int base, const f32x16& v) __attribute__((always_inline)) {
    if constexpr (FDMI_SA_DUMP != 0 && PROF) {
      if (blockIdx.x == 0 && wq == 0 && slot == FDMI_SA_DUMP && p.stamps != nullptr) {
        float* out = reinterpret_cast<float*>(p.stamps + 4 * 64 * 16);
#pragma unroll
        for (int r = 0; r < 16; ++r) out[(base + r) * 64 + lane] = v[r];
      }
    }
  };

  // ================================================================ projection: one stage = one k-tile of the head's 96 weight rows =
  // eighteen MFMAs in six groups of three (one per accumulator: consecutive MFMAs never share one; per accumulator the order of
  // gemm_img.hip, wh ah | wh al | wl ah per k16 step).  Two fragment buffers: X = the hi plane of the step, Y = its lo plane; the next
  // step's planes are requested right behind the last MFMA that reads the buffer, at least three MFMAs before their first use.
  f16x8 Xw[3], Yw[3];
  unsigned wb = 0;  // this lane's fragment base inside the stage being computed
  auto rd_w = [&](f16x8 (&dst)[3], int unit) __attribute__((always_inline)) {
#pragma unroll
    for (int j = 0; j < 3; ++j) dst[j] = __builtin_bit_cast(f16x8, lds_u128(wb + (unsigned)(unit * 1536 + j * 512)));
  };
  auto proj_first = [&]() __attribute__((always_inline)) {  // (the stream's very first stage; afterwards every stage finds its first planes in place)
    wb = w_rd + (unsigned)((pos & (NST - 1)) * KT_BYTES);
    rd_w(Xw, 0);
    rd_w(Yw, 4);
  };
  // MFMA k = 3 g + j of the stage: group g, accumulator j (q | k in the swapped form, v in the normal form: lane = feature).  The
  // planes of k16 step 0 of the NEXT stage (which has landed: see the stage-top wait) are requested as soon as X / Y are free, so a
  // stage's first MFMA does not wait for an LDS round trip behind the barrier.
  auto proj_mfma = [&](auto KT, auto K) __attribute__((always_inline)) {
    constexpr int kt = decltype(KT)::value, k = decltype(K)::value, g = k / 3, j = k % 3;
    if (FDMI_SA_DBG & 2) return;
    const f16x8& w = (g == 2 || g == 5) ? Yw[j] : Xw[j];
    const f16x8& hf = (g == 1 || g == 4) ? hl[kt][g / 3] : hh[kt][g / 3];
    if constexpr (j < 2) acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(w, hf, acc[j], 0, 0, 0);
    else acc[2] = __builtin_amdgcn_mfma_f32_32x32x16_f16(hf, w, acc[2], 0, 0, 0);
    if constexpr (k == 5) rd_w(Xw, 2);  // X is free: the hi plane of k16 step 1
    if constexpr (k == 8) rd_w(Yw, 6);  // Y is free: the lo plane of k16 step 1
    if constexpr (k == 14) {            // X is free: the next stage's hi plane of step 0
      wb = w_rd + (unsigned)(((pos + 1) & (NST - 1)) * KT_BYTES);
      rd_w(Xw, 0);
    }
    if constexpr (k == 17) rd_w(Yw, 4);  // Y is free: the next stage's lo plane of step 0
  };

  // ================================================================ the attention of one head, software pipelined into the 18 MFMA
  // slots of each of the twelve stages of the NEXT head's projection: slot k of the stage's slice is issued right behind projection
  // MFMA k, so an attention MFMA always has a projection MFMA between itself and the next one of its accumulator chain (a dependent
  // MFMA issues 64 cycles after its predecessor, an independent one after 32: with chunks of three dependent MFMAs between the
  // projection groups the fused stage took LONGER than the two kernels' stages together, profiles/r05_seq_attn_notes.log), and the
  // VALU / LDS work of a slot runs in the shadow of that MFMA.  The source order IS the schedule (sched_barrier between the pieces).
  //   stage 0       ctx block of the head before (normalise, split, store); then the head's projection epilogue: the three 32 x 32
  //                 accumulators (copied out at the stage's top) -> q_h operand registers, k_h -> LDS, v_h -> LDS
  //   stage 1 / 2   S^T tiles (0, 1) / (2, 3): the two tiles' MFMAs alternate
  //   stage 3       M0 M1 W0 W1          band tiles 0, 1: R^T = E Q^T (accumulators racc[0], racc[1]) and their scratch writes
  //   stage 4 5 6   M(s-2) G(s-4) W(s-2) the next band tile, the gather of pair s-4 into S^T tile T-1-(s-4), the tile's scratch write
  //   stage 7       G3, key mask, row maximum
  //   stage 8 / 9   exponentials of tiles (0, 1) / (2, 3), row sum
  //   stage 10 / 11 O^T += V^T P^T over key tiles (0, 1) / (2, 3)
  // (d_model 192: six stages, two slices each: the first slice in slots 0-8, two of its slots at a time, the second in slots 9-17.)
  f32x16 eo[3];          // the projected head's accumulators, copied out at the top of stage 0
  u32x4 kfa[4], kfb[4];  // K fragments of two S^T tiles / the table rows of two band tiles: [hi c0, hi c1, lo c0, lo c1]
  float gth[16];         // gathered band values
  float psum = 0.f;
  f16x8 pvh[2], pvl[2], pph[2], ppl[2];  // V^T and P operands of the P V triple in flight and of the next one
  u32x4 ch0, ch1, cl0, cl1;  // the packed ctx block
  float co[16];              // ... and its values
  unsigned eHh[4][2], eLo[4][2];  // split halves of the epilogue block being assembled
  int a_head = 0, c_head = 0, c_row0 = 0, c_nrows = 0;  // head of the attention in flight; (head, first row, rows) of the ctx block that leaves in stage 2

  auto split_quad = [&](auto Q, const float (&o)[4]) __attribute__((always_inline)) {
    constexpr int q = decltype(Q)::value;
    split_pair(o[0], o[1], eHh[q][0], eLo[q][0]);
    split_pair(o[2], o[3], eHh[q][1], eLo[q][1]);
  };
  // quad layout (lane half h owns d = 8 q + 4 h + e) -> MFMA operand layout (lane half h owns units 2 c + h: d = 16 c + 8 h + 0..7):
  // the half-waves exchange quad 1 of the lower against quad 0 of the upper lanes, and quad 3 against quad 2
  auto quad_to_operand = [&](unsigned (&X)[4][2]) __attribute__((always_inline)) {
#pragma unroll
    for (int dd = 0; dd < 2; ++dd) {
      swap32(X[0][dd], X[1][dd]);
      swap32(X[2][dd], X[3][dd]);
    }
  };
  // epilogue of the projected head `ph`, piece by piece (same arithmetic as gemm_img.hip's q | k and v^T epilogues):
  // the head's bias values are requested a few slots ahead of their first use (read at the point of use, every quad waited ~150
  // cycles for its LDS round trip: stage 0 took 3.8 k cycles, profiles/r05_seq_attn_notes.log)
  u32x4 bqk[2][4];  // [q | k][quad]: this lane's four bias values of the quad, at the image's scale
  float bvv = 0.f;
  auto bias_reads = [&](auto J, int ph) __attribute__((always_inline)) {  // J: 0 q, 1 k, 2 v
    constexpr int j = decltype(J)::value;
    int ln;  // (an opaque copy of the lane index: see ctx_store)
    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(ln));
    // (read through integer LDS addresses: behind a pointer derived from `smem` hipcc assumes that the read may alias the LDS-DMA
    // writes in flight and waits for the whole weight stream to land)
    if constexpr (j < 2) {
#pragma unroll
      for (int q = 0; q < 4; ++q) bqk[j][q] = lds_u128(par_base + (unsigned)((j * D + ph * 32 + 8 * q) * 4) + (unsigned)((ln >> 5) * 16));
    } else {
      bvv = lds_f32(par_base + (unsigned)((2 * D + ph * 32) * 4) + (unsigned)((ln & 31) * 4));
    }
  };
  auto epi_qk_quad = [&](auto J, auto Q) __attribute__((always_inline)) {  // J: 0 q, 1 k; quad Q of the lane's 16 features
    constexpr int j = decltype(J)::value, q = decltype(Q)::value;
    const float oss = j == 0 ? oss_q : oss_k;
    float o[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = __builtin_fmaf(eo[j][4 * q + e], oss, __builtin_bit_cast(float, (unsigned)bqk[j][q][e]));
    split_quad(Q, o);
  };
  auto epi_q_finish = [&]() __attribute__((always_inline)) {
    quad_to_operand(eHh);
    quad_to_operand(eLo);
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      qh[c] = __builtin_bit_cast(f16x8, u32x4{eHh[2 * c][0], eHh[2 * c][1], eHh[2 * c + 1][0], eHh[2 * c + 1][1]});
      ql[c] = __builtin_bit_cast(f16x8, u32x4{eLo[2 * c][0], eLo[2 * c][1], eLo[2 * c + 1][0], eLo[2 * c + 1][1]});
    }
  };
  auto epi_k_finish = [&]() __attribute__((always_inline)) {  // this lane's key is row 32 wq + l31 of the K tile; unit u at position u ^ (piece & 1)
    quad_to_operand(eHh);
    quad_to_operand(eLo);
    typedef __attribute__((address_space(3))) u32x4* lds_u128_t;
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      *(lds_u128_t)(unsigned long long)(k_wr + (unsigned)(2 * c * 128)) =
          u32x4{eHh[2 * c][0], eHh[2 * c][1], eHh[2 * c + 1][0], eHh[2 * c + 1][1]};
      *(lds_u128_t)(unsigned long long)(k_wr + (unsigned)((4 + 2 * c) * 128)) =
          u32x4{eLo[2 * c][0], eLo[2 * c][1], eLo[2 * c + 1][0], eLo[2 * c + 1][1]};
    }
  };
  // v (normal form): lane = feature d = l31, register r = 4 q + e <-> key 8 q + 4 half + e of the wave's key block: a quad is one
  // 8-byte unit 2 q + half of the block's feature row (hi), + 8 (lo), stored at unit ^ vt_swz(d)
  auto epi_v_quad = [&](auto Q) __attribute__((always_inline)) {
    constexpr int q = decltype(Q)::value;
    const float bz = bvv;
    const float o[4] = {__builtin_fmaf(eo[2][4 * q + 0], oss_v, bz), __builtin_fmaf(eo[2][4 * q + 1], oss_v, bz),
                        __builtin_fmaf(eo[2][4 * q + 2], oss_v, bz), __builtin_fmaf(eo[2][4 * q + 3], oss_v, bz)};
    split_quad(Q, o);
    typedef __attribute__((address_space(3))) u32x2* lds_u64_t;
    *(lds_u64_t)(unsigned long long)(v_wr + (unsigned)(((2 * q + half) ^ vsz) << 3)) = u32x2{eHh[q][0], eHh[q][1]};
    *(lds_u64_t)(unsigned long long)(v_wr + (unsigned)(((2 * q + half + 8) ^ vsz) << 3)) = u32x2{eLo[q][0], eLo[q][1]};
  };
  // ctx[token row][head block] = O^T[d][query] / l_run at the ctx image's scale (attention_img.hip: flush_ctx)
  auto ctx_scale_block = [&]() __attribute__((always_inline)) {
    const float onorm = p.ctx_scale / (p.v_scale * l_run);
#pragma unroll
    for (int r = 0; r < 16; ++r) co[r] = oacc[r] * onorm;
    if constexpr (FDMI_SA_DUMP != 0 && PROF) {  // (the ctx block of the dumped attention leaves one iteration later)
      if (blockIdx.x == 0 && wq == 0 && slot == FDMI_SA_DUMP + 1 && p.stamps != nullptr) {
        float* out = reinterpret_cast<float*>(p.stamps + 4 * 64 * 16);
#pragma unroll
        for (int r = 0; r < 16; ++r) out[(240 + r) * 64 + lane] = oacc[r];
        out[256 * 64 + lane] = l_run;
      }
    }
  };
  auto ctx_store = [&]() __attribute__((always_inline)) {
    // (the lane indices are re-derived from an opaque copy: as values that live across the whole loop one of their derivatives was
    // spilled, and its scratch reload -- a vector-memory load -- drained the weight stream once per iteration)
    int ln;
    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(ln));
    const int l = 32 * wq + (ln & 31);
    const int row = c_row0 + l;
    unsigned voff = (unsigned)((((row >> 5) * H * 8 + 2 * (ln >> 5)) * 32 + (row & 31)) * 16);
    voff = l < c_nrows ? voff : 0xFFFFFF00u;
    const int hoff = c_head * 4096;
    const __amdgpu_buffer_rsrc_t rsc = __builtin_amdgcn_make_buffer_rsrc(p.ctx, 0, 0xFFFFFF00u, 0x00020000);
    if (!(FDMI_SA_DBG & 4)) {
      __builtin_amdgcn_raw_buffer_store_b128(ch0, rsc, (int)voff, hoff, 0);
      __builtin_amdgcn_raw_buffer_store_b128(ch1, rsc, (int)voff, hoff + 512, 0);
      __builtin_amdgcn_raw_buffer_store_b128(cl0, rsc, (int)voff, hoff + 4 * 512, 0);
      __builtin_amdgcn_raw_buffer_store_b128(cl1, rsc, (int)voff, hoff + 5 * 512, 0);
      store_guard(ch0, ch1);
      store_guard(cl0, cl1);
    }
  };

  auto k_reads = [&](auto TT, auto CC, u32x4 (&kf)[4]) __attribute__((always_inline)) {  // K fragments (hi, lo) of tile t, k16 step c
    constexpr int t = decltype(TT)::value, c = decltype(CC)::value;
    kf[c] = lds_u128(k_rd + (unsigned)(t * 4096 + 2 * c * 128));
    kf[2 + c] = lds_u128(k_rd + (unsigned)(t * 4096 + (4 + 2 * c) * 128));
  };
  // MFMA i (0..5) of S^T tile t: k16 step i / 3, then kh qh | kh ql | kl qh
  auto s_mm1 = [&](auto TT, auto I, const u32x4 (&kf)[4]) __attribute__((always_inline)) {
    constexpr int t = decltype(TT)::value, i = decltype(I)::value, c = i / 3, j = i % 3;
    const f16x8 a = __builtin_bit_cast(f16x8, kf[j == 2 ? 2 + c : c]);
    const f16x8& b = j == 1 ? ql[c] : qh[c];
    if constexpr (i == 0) mfma_new(sacc[t], a, b);
    else mfma_acc(sacc[t], a, b);
    if constexpr (i == 5 && !FDMI_SA_ASM_MFMA) asm volatile("" : "+v"(sacc[t]));
  };
  auto e_reads = [&](auto QQ, u32x4 (&e)[4]) __attribute__((always_inline)) {  // e[0] hi c0, e[1] hi c1, e[2] lo c0, e[3] lo c1 of the lane's band row
    constexpr int qq = decltype(QQ)::value;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
#ifdef FDMI_SA_OLD_E
      const int rp = p.maxpos - LP + esh + 32 * wq + pi31;
      e[k] = lds_u128(a_Es + (unsigned)(rp * 128 + (((2 * k + half) ^ ((rp >> 1) & 7)) << 4)) + (unsigned)(qq * 4096));
#else
      e[k] = lds_u128((eaddr0 ^ (unsigned)(32 * k)) + (unsigned)(qq * 4096));
#endif
    }
  };
  // MFMA i (0..5) of R^T tile qq (rows = band rows pi(i), columns = this wave's queries) -> racc[qq & 1]: eh qh | el qh | eh ql per k16 step
  auto m_mm1 = [&](auto QQ, auto I, const u32x4 (&e)[4]) __attribute__((always_inline)) {
    constexpr int qq = decltype(QQ)::value, i = decltype(I)::value, c = i / 3, j = i % 3;
    const f16x8 a = __builtin_bit_cast(f16x8, e[j == 1 ? 2 + c : c]);
    const f16x8& b = j == 2 ? ql[c] : qh[c];
    if constexpr (i == 0) mfma_new(racc[qq & 1], a, b);
    else mfma_acc(racc[qq & 1], a, b);
    if constexpr (i == 5 && !FDMI_SA_ASM_MFMA) asm volatile("" : "+v"(racc[qq & 1]));
  };
  auto op_W = [&](auto QQ) __attribute__((always_inline)) {  // scratch slot qq & 1 <- racc[qq & 1]: register r of all 64 lanes lands as band rows 2 r, 2 r + 1
    constexpr int qq = decltype(QQ)::value;
    const f32x16 ra = racc[qq & 1];
    const unsigned m0v = rw_lds + (unsigned)((qq & 1) * 4096);
    unsigned keep;
    asm volatile(
        "s_nop 7\n\ts_mov_b32 %0, m0\n\ts_mov_b32 m0, %17\n\ts_nop 2\n\t"
        "ds_write_addtid_b32 %1 offset:0\n\tds_write_addtid_b32 %2 offset:256\n\t"
        "ds_write_addtid_b32 %3 offset:512\n\tds_write_addtid_b32 %4 offset:768\n\t"
        "ds_write_addtid_b32 %5 offset:1024\n\tds_write_addtid_b32 %6 offset:1280\n\t"
        "ds_write_addtid_b32 %7 offset:1536\n\tds_write_addtid_b32 %8 offset:1792\n\t"
        "ds_write_addtid_b32 %9 offset:2048\n\tds_write_addtid_b32 %10 offset:2304\n\t"
        "ds_write_addtid_b32 %11 offset:2560\n\tds_write_addtid_b32 %12 offset:2816\n\t"
        "ds_write_addtid_b32 %13 offset:3072\n\tds_write_addtid_b32 %14 offset:3328\n\t"
        "ds_write_addtid_b32 %15 offset:3584\n\tds_write_addtid_b32 %16 offset:3840\n\t"
        "s_mov_b32 m0, %0"
        : "=&s"(keep)
        : "v"(ra[0]), "v"(ra[1]), "v"(ra[2]), "v"(ra[3]), "v"(ra[4]), "v"(ra[5]), "v"(ra[6]), "v"(ra[7]),
          "v"(ra[8]), "v"(ra[9]), "v"(ra[10]), "v"(ra[11]), "v"(ra[12]), "v"(ra[13]), "v"(ra[14]), "v"(ra[15]),
          "s"(m0v)
        : "memory");
  };
  // S^T tile T-1-q += r_scale * band value of the tile pair (q, q+1): one ds_read_b32 and one fma per score
  auto g_reads = [&](auto Q) __attribute__((always_inline)) {
    constexpr int q = decltype(Q)::value;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int klr = (r & 3) + 8 * (r >> 2);
      if constexpr ((q & 1) == 0) gth[r] = lds_f32(gb + (unsigned)((27 - klr) * 128));
      else gth[r] = lds_f32(rw_base | ((gwrap + (unsigned)((27 - klr) * 128)) & 8191u));
    }
  };
  auto g_fma4 = [&](auto Q, auto R0) __attribute__((always_inline)) {
    constexpr int t = T - 1 - decltype(Q)::value, r0 = decltype(R0)::value;
#pragma unroll
    for (int r = r0; r < r0 + 4; ++r) {
      float f = __builtin_fmaf(gth[r], p.r_scale, sacc[t][r]);
      asm volatile("" : "+v"(f));  // (keeps the fma in this slot, see exp_range)
      sacc[t][r] = f;
    }
  };
  // exponentials of elements [lo, hi) of the 32 scores of tiles (tbase, tbase + 1), summed in element order
  auto exp_range = [&](int tbase, int lo, int hi) __attribute__((always_inline)) {
#pragma unroll
    for (int e = 0; e < 32; ++e) {
      if (e < lo || e >= hi) continue;
      const int t = tbase + (e >> 4), r = e & 15;
      const float pexp = exp2_neg(__builtin_fmaf(sacc[t][r], s_scale, nm));
      sacc[t][r] = pexp;
      psum += pexp;
    }
    // (a use with side effects in THIS slot: a pure chain whose first use sits in a later stage is sunk there -- the exponentials of
    // tiles 0, 1 all ran at the top of the next stage)
    asm volatile("" : "+v"(psum));
  };
  // P V over key tile t, k16 step c: operands (split of eight probabilities, four 8-byte V^T units) into buffer g & 1 of unit
  // g = 2 t + c, prepared while the unit before it multiplies; then vh ph | vl ph | vh pl
  auto pv_prep = [&](auto G) __attribute__((always_inline)) {
    constexpr int g = decltype(G)::value, t = g / 2, c = g % 2, bf = g & 1;
    u32x4 phu, plu;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      unsigned hv, lv;
      split_pair(sacc[t][8 * c + 2 * j], sacc[t][8 * c + 2 * j + 1], hv, lv);
      phu[j] = hv;
      plu[j] = lv;
    }
    pph[bf] = __builtin_bit_cast(f16x8, phu);
    ppl[bf] = __builtin_bit_cast(f16x8, plu);
    typedef const __attribute__((address_space(3))) u32x2* lds_cu64_t;
    const unsigned blk = v_rd + (unsigned)(t * 4096);
    const int ua = 4 * c + half;
    const u32x2 vh0 = *(lds_cu64_t)(unsigned long long)(blk + (unsigned)((ua ^ vsz) << 3));
    const u32x2 vh1 = *(lds_cu64_t)(unsigned long long)(blk + (unsigned)(((ua + 2) ^ vsz) << 3));
    const u32x2 vl0 = *(lds_cu64_t)(unsigned long long)(blk + (unsigned)(((ua + 8) ^ vsz) << 3));
    const u32x2 vl1 = *(lds_cu64_t)(unsigned long long)(blk + (unsigned)(((ua + 10) ^ vsz) << 3));
    pvh[bf] = __builtin_bit_cast(f16x8, u32x4{vh0[0], vh0[1], vh1[0], vh1[1]});
    pvl[bf] = __builtin_bit_cast(f16x8, u32x4{vl0[0], vl0[1], vl1[0], vl1[1]});
  };
  auto pv_mm1 = [&](auto G, auto J) __attribute__((always_inline)) {  // J: 0 vh ph | 1 vl ph | 2 vh pl
    constexpr int g = decltype(G)::value, j = decltype(J)::value, bf = g & 1;
    const f16x8& a = j == 1 ? pvl[bf] : pvh[bf];
    const f16x8& b = j == 2 ? ppl[bf] : pph[bf];
    if constexpr (g == 0 && j == 0) mfma_new(oacc, a, b);
    else mfma_acc(oacc, a, b);
    if constexpr (g == 7 && j == 2 && !FDMI_SA_ASM_MFMA) asm volatile("" : "+v"(oacc));
  };

  // slot k (0..17; -1: in front of the stage's first projection MFMA) of attention slice s.  `ph`: the head whose projection
  // finished in the previous iteration (its epilogue is slice 0)
  auto attn_slot = [&](auto S, auto K, int ph) __attribute__((always_inline)) {
    constexpr int s = decltype(S)::value, k = decltype(K)::value;
    if (FDMI_SA_DBG & 1) return;
    if constexpr (((FDMI_SA_SKIP >> s) & 1) != 0) return;
    if constexpr (s == 0) {
      // (q and k here: the S^T tiles of the next stage want them; v and the ctx block of the head before ride in the two S^T
      // stages, which are light on VALU work)
      if constexpr (k == -1) {
        bias_reads(IC<0>{}, ph);
        dump16(0, eo[0]); dump16(16, eo[1]); dump16(32, eo[2]);
      }
      if constexpr (k == 0) bias_reads(IC<1>{}, ph);
      if constexpr (k == 1) bias_reads(IC<2>{}, ph);
      if constexpr (k >= 2 && k <= 5) epi_qk_quad(IC<0>{}, IC<(k >= 2 && k <= 5) ? k - 2 : 0>{});
      if constexpr (k == 6) epi_q_finish();
      if constexpr (k >= 8 && k <= 11) epi_qk_quad(IC<1>{}, IC<(k >= 8 && k <= 11) ? k - 8 : 0>{});
      if constexpr (k == 12) epi_k_finish();
    }
    if constexpr (s == 1 || s == 2) {
      constexpr int ta = 2 * (s - 1), tb = ta + 1;
      if constexpr (k == -1) { k_reads(IC<ta>{}, IC<0>{}, kfa); k_reads(IC<tb>{}, IC<0>{}, kfb); }
      if constexpr (k == 1) { k_reads(IC<ta>{}, IC<1>{}, kfa); k_reads(IC<tb>{}, IC<1>{}, kfb); }
      if constexpr (k >= 2 && k <= 13) {
        constexpr int i = (k >= 2 && k <= 13) ? (k - 2) / 2 : 0;
        if constexpr ((k & 1) == 0) s_mm1(IC<ta>{}, IC<i>{}, kfa);
        else s_mm1(IC<tb>{}, IC<i>{}, kfb);
      }
      if constexpr (s == 1) {  // the v part of the projection epilogue (V^T is not read before stage 10)
        if constexpr (k == 4 || k == 8 || k == 12 || k == 16) epi_v_quad(IC<(k == 4 || k == 8 || k == 12 || k == 16) ? k / 4 - 1 : 0>{});
      }
      if constexpr (s == 2) {  // the ctx block of the head before
        if constexpr (k == 0) ctx_scale_block();
        if constexpr (k == 6) pack_block(co, 1.0f, ch0, ch1, cl0, cl1);
        if constexpr (k == 12) ctx_store();
      }
    }
    if constexpr (s == 3) {
      if constexpr (k == -1) {
        e_reads(IC<0>{}, kfa); e_reads(IC<1>{}, kfb);
        dump16(48, sacc[0]); dump16(64, sacc[1]); dump16(80, sacc[2]); dump16(96, sacc[3]);  // raw S^T
      }
      if constexpr (k >= 2 && k <= 13) {
        constexpr int i = (k >= 2 && k <= 13) ? (k - 2) / 2 : 0;
        if constexpr ((k & 1) == 0) m_mm1(IC<0>{}, IC<i>{}, kfa);
        else m_mm1(IC<1>{}, IC<i>{}, kfb);
      }
      if constexpr (k == 15) op_W(IC<0>{});
      if constexpr (k == 17) op_W(IC<1>{});
    }
    if constexpr (s >= 4 && s <= 6) {
      constexpr int m = s - 2, q = s - 4;
      if constexpr (k == -1) { e_reads(IC<m>{}, kfa); g_reads(IC<q>{}); }
      if constexpr (k >= 2 && k <= 7) m_mm1(IC<m>{}, IC<(k >= 2 && k <= 7) ? k - 2 : 0>{}, kfa);
      if constexpr (k >= 8 && k <= 11) g_fma4(IC<q>{}, IC<(k >= 8 && k <= 11) ? 4 * (k - 8) : 0>{});
      if constexpr (k == 14) op_W(IC<m>{});
    }
    if constexpr (s == 7) {
      if constexpr (k == -1) g_reads(IC<3>{});
      if constexpr (k >= 2 && k <= 5) g_fma4(IC<3>{}, IC<(k >= 2 && k <= 5) ? 4 * (k - 2) : 0>{});
      if constexpr (k == 6) {
        dump16(112, sacc[0]); dump16(128, sacc[1]); dump16(144, sacc[2]); dump16(160, sacc[3]);  // S^T with the band
        // key mask: this lane + its partner (lane ^ 32) hold one query's scores
        // (len <= Lb: a key tile that ends at or below len has nothing to mask; len is wave-uniform, and this slot is a block of
        // its own anyway -- sequences of 97..128 positions touch the last tile only)
        if (len < LP) {
          static_for<0, T>([&](auto TT) __attribute__((always_inline)) {
            constexpr int t = decltype(TT)::value;
            if (len < 32 * (t + 1)) {
#pragma unroll
              for (int r = 0; r < 16; ++r) {
                const int key = 32 * t + (r & 3) + 8 * (r >> 2) + 4 * half;
                float sc = sacc[t][r];
                if (key >= len) sc += mask_raw;  // (1 - mask) * -10000   (modelling.py:452)
                if (key >= Lb) sc = -INFINITY;   // not a key at all (rows that do not exist)
                sacc[t][r] = sc;
              }
            }
          });
        }
        mt = -INFINITY;
      }
      if constexpr (k >= 7 && k <= 14) {  // row maximum, eight scores per slot in element order
        constexpr int e0 = (k >= 7 && k <= 14) ? 8 * (k - 7) : 0;
        float m = mt;
#pragma unroll
        for (int e = e0; e < e0 + 8; ++e) m = fmaxf(m, sacc[e >> 4][e & 15]);
        asm volatile("" : "+v"(m));  // (keeps the maxima in this slot, see exp_range)
        mt = m;
      }
      if constexpr (k == 15) {
        mt = pair_max(mt);
        nm = __builtin_fmaf(-mt, s_scale, 10.0f);  // + log2(PS): p' = PS * 2^((u - m) * s_scale)
        static_assert(PS == 1024.0f, "exponent offset above is log2(PS)");
        psum = 0.f;
      }
    }
    if constexpr (s == 8 || s == 9) {
      if constexpr (k >= 0 && k <= 15) exp_range(2 * (s - 8), 2 * (k >= 0 ? k : 0), 2 * (k >= 0 ? k : 0) + 2);
      if constexpr (s == 9 && k == 16) l_run = pair_sum(psum);  // carries the factor PS
      if constexpr (s == 9 && k == 17) {
        dump16(176, sacc[0]); dump16(192, sacc[1]); dump16(208, sacc[2]); dump16(224, sacc[3]);  // probabilities
        pv_prep(IC<0>{});
      }
    }
    if constexpr (s == 10 || s == 11) {
      constexpr int g0 = 4 * (s - 10);  // units g0 .. g0 + 3: MFMAs in slots 4 u + 1 .. 4 u + 3, the next unit's operands prepared in slot 4 u + 1
      if constexpr (k >= 1 && k <= 16) {
        constexpr int kk = (k >= 1 && k <= 16) ? k - 1 : 0, u = kk / 4, j = kk % 4;
        if constexpr (j < 3) pv_mm1(IC<g0 + u>{}, IC<j>{});
        if constexpr (j == 0 && g0 + u + 1 < 8) pv_prep(IC<(g0 + u + 1 < 8) ? g0 + u + 1 : 0>{});
      }
    }
  };
  // the attention work behind projection MFMA `slot` of stage kt.  d_model 384: one slice per stage, slot = slice slot.  d_model 192
  // (six stages, two slices A, B per stage, NOT interleaved with each other: they share registers): slots 0-8 run A's slots two
  // at a time (its slot -1 in front of the stage), slots 9-17 run B's (its slot -1 with A's last).
  auto attn_at = [&](auto KT, auto SLOT, int ph) __attribute__((always_inline)) {
    constexpr int kt = decltype(KT)::value, slot = decltype(SLOT)::value;
    if constexpr (SPS == 1) {
      attn_slot(IC<kt>{}, IC<slot>{}, ph);
    } else {
      constexpr int a = 2 * kt, b = 2 * kt + 1;
      if constexpr (slot == -1) attn_slot(IC<a>{}, IC<-1>{}, ph);
      if constexpr (slot >= 0 && slot <= 8) { attn_slot(IC<a>{}, IC<2 * slot>{}, ph); attn_slot(IC<a>{}, IC<2 * slot + 1>{}, ph); }
      if constexpr (slot == 8) {
        // slices 0 and 1 share stage 0: the K tiles that every wave wrote in slice 0 are read by every wave in slice 1 (with the
        // projection's MFMAs pacing the slots the waves happened to stay ~2 slots apart; the attention-only last iteration showed
        // the race)
        if constexpr (kt == 0) barrier_keep_vm();
        attn_slot(IC<b>{}, IC<-1>{}, ph);
      }
      if constexpr (slot >= 9) { attn_slot(IC<b>{}, IC<2 * (slot - 9)>{}, ph); attn_slot(IC<b>{}, IC<2 * (slot - 9) + 1>{}, ph); }
    }
  };

  // ================================================================ the item stream.  Item i = (sequence i / H of this workgroup,
  // head i % H); iteration i runs the projection of item i fused with the attention of item i - 1 (whose epilogue opens it, and whose
  // ctx block leaves at the start of iteration i + 1) -- across sequences too: the hidden state of the next sequence replaces the
  // current one IN PLACE, k-tile by k-tile, each right behind its last use in the sequence's last head (twelve stages before its
  // first use).  Iteration 0's attention works on garbage (its stores are dropped: nrows = 0); the last iteration projects the last
  // head once more for nothing -- ONE loop body without branches around the MFMAs = one register allocation: with separate code for
  // the first / last head of a sequence hipcc moved ~200 registers through scratch at every seam (44 k cycles each,
  // profiles/r05_seq_attn_notes.log).
  int seq = blockIdx.x;
  if (seq >= p.B) {
    FD_WAIT_VM(0);
    return;
  }
  const int nitems = nseq * H;
  int p_row0 = p.seq_row0[seq];  // first row of the sequence being projected
  static_for<0, NKT>([&](auto KT) __attribute__((always_inline)) { load_h_kt(KT, p_row0); });
#pragma unroll
  for (int j = 0; j < 3; ++j) acc[j] = zero16;
  oacc = zero16;
  issue_w(IC<0>{});
  issue_w(IC<0>{});
  issue_w(IC<0>{});
  FD_WAIT_VM(6);  // the first stage (and the hidden state, requested before it) landed
  barrier_keep_vm();
  proj_first();
  int head = 0;       // head of the item being projected
  int prev_head = 0;  // ... of the item before it, whose attention this iteration runs
  int prev_seq = seq, prev_row0 = p_row0;
#if FDMI_SA_EDGES
  // ---- iteration 0: the projection of the first item alone (no attention slots: 12 stages of ~870 ticks instead of ~1660)
  static_for<0, NKT>([&](auto KT) __attribute__((always_inline)) {
    constexpr int kt = decltype(KT)::value;
    FD_STAMP(kt);
    FD_WAIT_VM(3);
    barrier_keep_vm();
    issue_w(IC<(kt == NKT - 3)>{});
    FD_SB();
    static_for<0, 18>([&](auto K) __attribute__((always_inline)) {
      proj_mfma(KT, K);
      FD_SB();
    });
    ++pos;
  });
  ++slot;
  head = 1;
  constexpr int IT0 = 1;
#else
  constexpr int IT0 = 0;
#endif
  const int it_end = FDMI_SA_EDGES ? nitems : nitems + 1;
  for (int it = IT0; it < it_end; ++it) {
    const bool real = FDMI_SA_EDGES ? true : it < nitems;
    // vector-memory bookkeeping of the stage-top waits: 0 plain (the 6 pieces of the two younger stages); 1 this iteration
    // re-loads the hidden state (4 more loads per stage); 2 the iteration after such a one
    const bool reload = real && head == H - 1 && seq + (int)gridDim.x < p.B;
    const int n_row0 = reload ? sload(p.seq_row0, seq + (int)gridDim.x) : 0;
    const bool after_reload = real && head == 0 && it > 0;
    // (one item in six; an opaque scalar, or hipcc takes the test apart again into the two it came from: the common case is then
    // one compare and one branch that is not taken per stage)
    int special = __builtin_amdgcn_readfirstlane((reload || after_reload) ? 1 : 0);
    asm volatile("" : "+s"(special));
    static_for<0, NKT>([&](auto KT) __attribute__((always_inline)) {
      constexpr int kt = decltype(KT)::value;
      FD_STAMP(kt);
      // the NEXT stage landed (this one did a stage ago).  vmcnt retires in issue order (loads and stores alike: the compiler's own
      // waits rest on that), so the stage is complete once no more operations are outstanding than were issued behind it: the 3
      // pieces of the stage after it, the 4 ctx stores of stage 2 (seen from the tops of stages 3 and 4), and -- while the hidden
      // state is being re-loaded -- the 4 loads issued at the end of the two stages before this one
      constexpr int ST = (SPS == 1 && (kt == 3 || kt == 4)) ? 4 : 0;  // (d_model 192: the stores leave in stage 1; the plain count only waits longer)
      if (__builtin_expect(special != 0, 0)) {
        if (reload) FD_WAIT_VM(3 + ST + (kt == 0 ? 0 : (kt == 1 ? 4 : 8)));
        else FD_WAIT_VM(3 + ST + (kt == 0 ? 8 : (kt == 1 ? 4 : 0)));
      } else {
        FD_WAIT_VM(3 + ST);
      }
      barrier_keep_vm();  // ... for every wave; every wave is done with the stage before: its slot is free
      if constexpr (kt == FDMI_SA_SUBSTAGE) FD_STAMP(15);  // (instrumented build: one stage in pieces -- barrier | copy-out, slot -1 | slots 0-6 | 7-12 | 13-17)
      issue_w(IC<(kt == NKT - 3)>{});
      if constexpr (kt == 0) {  // the finished head's accumulators leave the matrix registers: its epilogue runs under this stage
#pragma unroll
        for (int j = 0; j < 3; ++j) {
          eo[j] = acc[j];
          acc[j] = zero16;
        }
      }
      FD_SB();
      attn_at(KT, IC<-1>{}, prev_head);
      FD_SB();
      if constexpr (kt == FDMI_SA_SUBSTAGE) FD_STAMP(12);
      static_for<0, 18>([&](auto K) __attribute__((always_inline)) {
        proj_mfma(KT, K);
        if constexpr (FDMI_SA_SCHED == 0) FD_SB();
        attn_at(KT, K, prev_head);
        if constexpr (FDMI_SA_SCHED == 0) FD_SB();
        if constexpr (kt == FDMI_SA_SUBSTAGE && decltype(K)::value == 6) FD_STAMP(13);
        if constexpr (kt == FDMI_SA_SUBSTAGE && decltype(K)::value == 12) FD_STAMP(14);
      });
      if constexpr (FDMI_SA_SCHED != 0) {
        // behind every MFMA (their source order stands): a few VALU, one transcendental, two scalar, one LDS read, one LDS write
#pragma unroll
        for (int g = 0; g < 32; ++g) {
          __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
          __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
          __builtin_amdgcn_sched_group_barrier(0x002, FDMI_SA_SCHED, 0);
          __builtin_amdgcn_sched_group_barrier(0x400, 1, 0);
          __builtin_amdgcn_sched_group_barrier(0x004, 1, 0);
          __builtin_amdgcn_sched_group_barrier(0x200, 1, 0);
        }
        FD_SB();
      }
      if constexpr (kt == 0) {
        // the attention that starts now (item it - 1) may belong to a new sequence
        a_head = prev_head;
        if (prev_head == 0 && it > 0) {
          row0 = prev_row0;
          int r1;
          sload3(p.seq_row0, prev_seq + 1, p.nrow, prev_seq, p.lens, prev_seq, r1, Lb, len);
          nrows = r1 - row0;
        }
      }
      if constexpr (kt == (SPS == 1 ? 2 : 1)) {  // the ctx block of the head before has left: the next one belongs to the attention in flight
        c_head = a_head;
        c_row0 = row0;
        c_nrows = nrows;
      }
      if (reload) load_h_kt(KT, n_row0);
      FD_SB();
      ++pos;
    });
    ++slot;
    prev_head = head;
    prev_seq = seq;
    prev_row0 = p_row0;
    if (real && ++head == H) {
      head = 0;
      if (seq + (int)gridDim.x < p.B) {
        seq += (int)gridDim.x;
        p_row0 = n_row0;
      }
    }
  }
#if FDMI_SA_EDGES
  // ---- the attention of the last item alone: no projection, no weight stream (what the stream requested beyond its end lands in
  // free ring slots and is never read), the same barriers (K / V of the item travel between the waves through LDS)
  static_for<0, NKT>([&](auto KT) __attribute__((always_inline)) {
    constexpr int kt = decltype(KT)::value;
    FD_STAMP(kt);
    barrier_keep_vm();
    if constexpr (kt == 0) {
#pragma unroll
      for (int j = 0; j < 3; ++j) eo[j] = acc[j];
    }
    FD_SB();
    attn_at(KT, IC<-1>{}, prev_head);
    FD_SB();
    static_for<0, 18>([&](auto K) __attribute__((always_inline)) {
      attn_at(KT, K, prev_head);
      FD_SB();
    });
    if constexpr (kt == 0) {
      a_head = prev_head;
      if (prev_head == 0) {
        row0 = prev_row0;
        int r1;
        sload3(p.seq_row0, prev_seq + 1, p.nrow, prev_seq, p.lens, prev_seq, r1, Lb, len);
        nrows = r1 - row0;
      }
    }
    if constexpr (kt == (SPS == 1 ? 2 : 1)) {
      c_head = a_head;
      c_row0 = row0;
      c_nrows = nrows;
    }
    FD_SB();
  });
  ++slot;
#endif
  // the last item's ctx block
  c_head = a_head;
  c_row0 = row0;
  c_nrows = nrows;
  ctx_scale_block();
  pack_block(co, 1.0f, ch0, ch1, cl0, cl1);
  ctx_store();
  FD_WAIT_VM(0);  // nothing may land in LDS after the workgroup has exited
#undef FD_STAMP
#undef FD_SB
}

template <int NKT>
static bool launch(const SeqAttnArgs& p, hipStream_t s, int grid_cap, int* grid_used) {
  static LdsOptIn lds;  // (the whole LDS of a CU)
  if (!lds({reinterpret_cast<const void*>(&seq_attn_kernel<NKT, false>), reinterpret_cast<const void*>(&seq_attn_kernel<NKT, true>)}, SMEM))
    return false;
  const int grid = persistent_grid(p.B, grid_cap);
  if (grid_used) *grid_used = grid;
  if (p.stamps) hipLaunchKernelGGL((seq_attn_kernel<NKT, true>), dim3(grid), dim3(256), SMEM, s, p);
  else hipLaunchKernelGGL((seq_attn_kernel<NKT, false>), dim3(grid), dim3(256), SMEM, s, p);
  return hipGetLastError() == hipSuccess;
}

}  // namespace sa

// head size 32, d_model 384 / 192 (every released configuration / the reference's test fixture), a sequence = one tile of 128 keys
// with all four 32-key tiles in use, the distance table in 32 KiB of LDS
bool seq_attn_supported(int d_model, int n_heads, int L, int maxpos) {
  return (d_model == 384 || d_model == 192) && n_heads * 32 == d_model && L > 96 && L <= 128 && maxpos <= 128 && maxpos >= L;
}

bool launch_seq_attn(const SeqAttnArgs& p, hipStream_t s, int grid_cap, int* grid_used) {
  return p.H == 12 ? sa::launch<12>(p, s, grid_cap, grid_used) : sa::launch<6>(p, s, grid_cap, grid_used);
}

}  // namespace fdmi
