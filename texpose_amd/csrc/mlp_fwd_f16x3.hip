// K2 (fast path): fused posenc + static/transient/light MLP forward on the f16 matrix cores with
// fp32-grade accuracy ("f16x3").  Same interface, schedule and register-resident dataflow as
// mlp_fwd.hip; what changes is the arithmetic of each product:
//
//   gfx950 has no TF32/xf32, and v_mfma_f32_32x32x2_f32 runs at 1/16 of the f16 MFMA rate.  Here every
//   fp32 operand (weights offline, activations while the consuming layer's MFMAs issue) is carried as an unevaluated sum
//   hi + lo of two fp16 numbers (11 + 11 significand bits), and   W x  ~=  Whi xhi + Whi xlo + Wlo xhi
//   is issued as three v_mfma_f32_32x32x16_f16 with fp32 accumulation.  Products of two fp16 values are
//   exact in fp32, the dropped lo*lo term is 2^-22 relative, so the result is as accurate as an fp32
//   FMA chain (measured vs an fp64 oracle: within 1.3x of torch fp32) at 16/3 = 5.3x
//   the fp32-MFMA throughput.  Weights are pre-scaled by 2^8 (exact) so that their lo parts stay in the
//   fp16 normal range; the accumulators are seeded with bias * 2^8 and the 2^-8 is applied when they are converted.  Activations must stay below 6e4
//   (NeRF activations are O(1..100)); the kernel raises bit 0 of a status word otherwise.
//
// An accumulator tile is reused as the next layer's B operand exactly as in the fp32 kernel: registers
// 8s..8s+7 of a 32x32 tile, converted to fp16, ARE the B fragment of k-step s (rows 16s + 8(j>>2) + 4h + (j&3)),
// and the packed weights absorb that row permutation (mlp_layout.h, "f16x3 stream").
#include "mlp_mma.h"
#include "wide_asm.inc.h"
#include <type_traits>

namespace {
using namespace tp_layout;
using namespace tp_mma;

using half8 = __attribute__((ext_vector_type(8))) _Float16;
using half2v = __attribute__((ext_vector_type(2))) __fp16;

constexpr int kBiasPad = (kBiasFloats + 63) / 64 * 64;
constexpr int kStageHalves = 5 * 2 * kThreads * 8;             // 5 k-steps x (hi, lo) x 256 lanes x 8 halves = 40 KiB

constexpr int kBufs = 3;                                         // weight-chunk ring: two chunks (3072 cycles) ahead
constexpr int kSaveFloats = 8 * kThreads;                       // forward: 8 lane-private floats kept in LDS across the blocks
constexpr int kLdsBytes = kBufs * kChunkFloats * 4 + kBiasPad * 4 + kStageHalves * 2 + kSaveFloats * 4;
constexpr float kInvScale = 1.0f / (float)(1 << kF16WeightShift);

using u32x4 = __attribute__((ext_vector_type(4))) unsigned int;
__device__ __forceinline__ half8 pack8(const half2v (&p)[4]) {
  const u32x4 w = {__builtin_bit_cast(unsigned int, p[0]), __builtin_bit_cast(unsigned int, p[1]),
                   __builtin_bit_cast(unsigned int, p[2]), __builtin_bit_cast(unsigned int, p[3])};
  return __builtin_bit_cast(half8, w);
}

// Three-slot ring instead of the fp32 kernel's double buffer: a chunk is only 48 MFMAs (1536 cycles, ~0.65 us)
// here, shorter than an L2->LDS DMA round trip, so the prefetch runs TWO chunks ahead.  The DMA of chunk c+2 stays
// in flight across the barrier: counted `s_waitcnt vmcnt(n)` (the n DMA instructions of the newest chunk issued so
// far may be outstanding, everything older -- chunk c+1 -- has landed) + raw s_barrier; __syncthreads() would drain
// vmcnt(0).
//
// The A-fragment fetch (LDS -> VGPR, kDepth pairs ahead of the MFMAs that use them) is ONE continuous pipeline
// across chunks: the barrier that publishes chunk c+1 sits kDepth pairs before the END of chunk c, and the last
// iterations of chunk c already fetch the first pairs of chunk c+1.  With one wave per SIMD nothing else would hide
// the LDS latency of a per-chunk prologue.  Slot safety: the DMA issued at the start of chunk c+1 (chunk c+3)
// overwrites the slot of chunk c, and every wave has completed (lgkmcnt(0)) all its reads of chunk c before it
// arrives at chunk c's barrier, which every wave passes before it starts chunk c+1.  The generated blocks of
// wide_asm.inc.h run this protocol; the compiled code only primes the ring at kernel start (frag_prime).
constexpr int kDepth = 4;
constexpr int kPairHalves = 1024;                  // one (k-step, tile) pair: 512 halves hi + 512 halves lo
struct Frag { half8 h[kDepth], l[kDepth]; };

#ifdef TP_TRACE
__device__ __forceinline__ long long tick() {
  long long t;
  asm volatile("s_memtime %0\n s_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
  return t;
}
#define TR_BEGIN(a) const long long tr_##a = tick()
#define TR_END(k, a) p.tr[k] += tick() - tr_##a
#else
// product build: the section marks stay compiler fences.  They keep hipcc from moving LDS / memory operations of
// one section into another (e.g. hoisting a staging section's loads across a head), which lengthens live ranges
// past what the 512-register budget next to two accumulator sets allows and ends in scratch spills.
#define TR_BEGIN(a) asm volatile("" ::: "memory")
#define TR_END(k, a) asm volatile("" ::: "memory")
#endif

__device__ __forceinline__ const _Float16* chunk_ptr16(const Pipe& p) {
  return reinterpret_cast<const _Float16*>(p.lds + p.buf * kChunkFloats) + p.lane * 8;
}
__device__ __forceinline__ void frag_fetch(Frag& f, int slot, const _Float16* src) {
  f.h[slot] = *reinterpret_cast<const half8*>(src);
  f.l[slot] = *reinterpret_cast<const half8*>(src + 512);
}
// pairs 0..kDepth-1 of the current chunk (kernel start only; afterwards the pipeline never drains)
__device__ __forceinline__ void frag_prime(const Pipe& p, Frag& f) {
  const _Float16* l = chunk_ptr16(p);
#pragma unroll
  for (int q = 0; q < kDepth; ++q) frag_fetch(f, q, l + q * kPairHalves);
}

// range guard: running maximum of the packed hi halves (v_pk_max_f16, two elements per instruction).  Round-to-zero
// conversion saturates at 65504, so "amax >= 6e4" still detects every out-of-range activation.
struct Guard { half2v m = {(__fp16)0.0f, (__fp16)0.0f}; };

__device__ __forceinline__ float softplus(float x) { return x > 20.0f ? x : log1pf(expf(x)); }
__device__ __forceinline__ float sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }


// =====================================================================================================================
// Everything that touches the two accumulator sets -- in the forward kernels and in the data gradient further down -- runs
// in the hand-scheduled asm blocks of wide_asm.inc.h (generated by gen_wide_asm.py; the register map and the ring protocol
// are documented there): set P is pinned to a[0:127], set Q to a[128:255], the fragment ring to v[160:191].  The C++ around
// them stages inputs, applies the output non-linearities and stores.
// =====================================================================================================================
struct AsmCtx { unsigned lane16, laneoff, ldswave, stream_lo, stream_hi, bias0, stage0; int nch; };
// The context is RE-DERIVED from the hardware thread id at every block instead of being carried in registers: the compiler
// owns ~40 VGPRs while the trunk feature is stashed, and seven context values kept live across the whole tile loop went to
// scratch memory (whose lines, re-read every tile, then competed with the 3.6 MiB weight stream for the 4 MiB L2).  The
// empty volatile asm makes each derivation opaque, so nothing of it is hoisted or shared between blocks.
__device__ __forceinline__ AsmCtx asm_ctx_now(const float* packed, int nch = kNumChunks) {
  extern __shared__ __attribute__((aligned(16))) float lds_base[];
  int tid = threadIdx.x;
  asm volatile("" : "+v"(tid));
  const unsigned lane = (unsigned)tid & 63u, hh = ((unsigned)tid >> 5) & 1u;
  const unsigned wave = (unsigned)__builtin_amdgcn_readfirstlane(tid >> 6);
  AsmCtx c;
  const unsigned lds0 = (unsigned)(uintptr_t)AS3(lds_base);
  c.lane16 = lds0 + lane * 16u;
  c.laneoff = lane * 16u;
  c.ldswave = lds0 + wave * 8192u;
  const uint64_t sw = (uint64_t)(uintptr_t)(packed + wave * 2048);
  c.stream_lo = (unsigned)sw;
  c.stream_hi = (unsigned)(sw >> 32);
  const unsigned bias_lds = lds0 + (unsigned)(kBufs * kChunkFloats) * 4u;
  c.bias0 = bias_lds + hh * 512u;                                          // + li * 1024: bias block of wide layer li
  c.stage0 = bias_lds + (unsigned)kBiasPad * 4u + (unsigned)tid * 16u;     // + ks * 8192: staged k-step ks (hi; lo at + 4096)
  c.nch = nch;                                                             // chunks in the stream the blocks walk (a constant at every call site)
  return c;
}
#define TP_RING(f)                                                                                                     \
  "+{v[160:163]}"(f.h[0]), "+{v[164:167]}"(f.l[0]), "+{v[168:171]}"(f.h[1]), "+{v[172:175]}"(f.l[1]),                  \
      "+{v[176:179]}"(f.h[2]), "+{v[180:183]}"(f.l[2]), "+{v[184:187]}"(f.h[3]), "+{v[188:191]}"(f.l[3])
#define TP_RING_STATE                                                                                                  \
  [chunk] "+s"(chunk), [buf] "+s"(buf), [r0] "=&s"(r0), [r1] "=&s"(r1), [r2] "=&s"(r2), [m0a] "=&s"(m0a),              \
      [m1a] "=&s"(m1a), [m2a] "=&s"(m2a), [dch] "=&s"(dch), [t0] "=&s"(t0)
#define TP_RING_INPUTS(c)                                                                                              \
  [lane16] "v"(c.lane16), [laneoff] "v"(c.laneoff), [ldswave] "s"(__builtin_amdgcn_readfirstlane(c.ldswave)),         \
      [stream_lo] "s"(__builtin_amdgcn_readfirstlane(c.stream_lo)),                                                    \
      [stream_hi] "s"(__builtin_amdgcn_readfirstlane(c.stream_hi)), [nch] "s"(c.nch)
#define TP_ASM_HACC "v232", "v233", "v234", "v235", "v236", "v237", "v238", "v239", "v240", "v241", "v242", "v243", "v244", "v245", "v246", "v247"
#define TP_RING_LOCALS                                                                                                 \
  int chunk = __builtin_amdgcn_readfirstlane(p.chunk), buf = __builtin_amdgcn_readfirstlane(p.buf);                    \
  int r0, r1, r2, m0a, m1a, m2a, dch, t0
#define TP_RING_DONE                                                                                                   \
  p.chunk = chunk;                                                                                                     \
  p.buf = buf

// The sets are NOT C++ values: the blocks address a[0:255] directly and the compiled code in between must never touch
// an AGPR (check_asm_ownership.py verifies that on the generated assembly; "a0" / "a255" in the clobber lists make the
// kernel allocate all 256).  Stash / restore of the trunk feature (set Q after L7 -> 128 VGPR values -> set P before R0):
#define TP_SF_OUT(F)                                                                                                   \
  "={v[32:47]}"(F[0]), "={v[48:63]}"(F[1]), "={v[64:79]}"(F[2]), "={v[80:95]}"(F[3]), "={v[96:111]}"(F[4]),            \
      "={v[112:127]}"(F[5]), "={v[128:143]}"(F[6]), "={v[144:159]}"(F[7])
#define TP_SF_IN(F)                                                                                                    \
  "{v[32:47]}"(F[0]), "{v[48:63]}"(F[1]), "{v[64:79]}"(F[2]), "{v[80:95]}"(F[3]), "{v[96:111]}"(F[4]),                 \
      "{v[112:127]}"(F[5]), "{v[128:143]}"(F[6]), "{v[144:159]}"(F[7])
__device__ __forceinline__ void asm_stash_q(f32x16 (&F)[8]) { asm volatile(TP_ASM_STASH_Q : TP_SF_OUT(F) : : TP_ASM_ALL_AGPRS); }
__device__ __forceinline__ void asm_restore_p(const f32x16 (&F)[8]) { asm volatile(TP_ASM_RESTORE_P : : TP_SF_IN(F) : TP_ASM_ALL_AGPRS); }
// 256 -> 256 layer body; SRC_Q: read set Q, accumulate into set P, else the reverse
template <bool SRC_Q>
__device__ __forceinline__ void asm_wide(Pipe& p, Frag& f, Guard& amax, const AsmCtx& c, int next_li) {
  TP_RING_LOCALS;
  const float kinv = kInvScale;
  const unsigned mask = 0xFFFFE000u;
  const unsigned nbias = c.bias0 + (unsigned)next_li * 1024u;       // the source set is re-seeded for the next layer
  if constexpr (SRC_Q)
    asm volatile(TP_ASM_WIDE_QP : TP_RING(f), TP_RING_STATE, [amax] "+v"(amax.m)
                 : TP_RING_INPUTS(c), [kinv] "s"(kinv), [mask] "s"(mask), [nbias] "v"(nbias)
                 : TP_ASM_CLOBBERS, TP_ASM_HACC, "memory", "scc");
  else
    asm volatile(TP_ASM_WIDE_PQ : TP_RING(f), TP_RING_STATE, [amax] "+v"(amax.m)
                 : TP_RING_INPUTS(c), [kinv] "s"(kinv), [mask] "s"(mask), [nbias] "v"(nbias)
                 : TP_ASM_CLOBBERS, TP_ASM_HACC, "memory", "scc");
  TP_RING_DONE;
}

// single-product arithmetic (TP_MLP_F16, gen_wide_asm.py "SINGLE PRODUCT"): the same layer on the f16 stream, 4 chunks of 32 MFMAs
template <bool SRC_Q>
__device__ __forceinline__ void asm_wide16(Pipe& p, Frag& f, Guard& amax, const AsmCtx& c, int next_li) {
  TP_RING_LOCALS;
  const unsigned nbias = c.bias0 + (unsigned)next_li * 1024u;
  if constexpr (SRC_Q)
    asm volatile(TP_ASM_WIDE16_QP : TP_RING(f), TP_RING_STATE, [amax] "+v"(amax.m)
                 : TP_RING_INPUTS(c), [nbias] "v"(nbias) : TP_ASM_CLOBBERS, "memory", "scc");
  else
    asm volatile(TP_ASM_WIDE16_PQ : TP_RING(f), TP_RING_STATE, [amax] "+v"(amax.m)
                 : TP_RING_INPUTS(c), [nbias] "v"(nbias) : TP_ASM_CLOBBERS, "memory", "scc");
  TP_RING_DONE;
}

// ---- recording variants (training): the block that CONSUMES a layer's accumulators also writes its activation record
// (gen_wide_asm.py, "recording variants").  Addresses of this lane in the wave's private 4 KB staging tile -- the wave's OWN
// slices of the first four 4 KB blocks of the input stage, dead while a WIDE / HEAD block runs -- and in the record block.
struct RecCtx { unsigned recw, recr, ro0, ro1, mkoff; const float* rbase; };
__device__ __forceinline__ RecCtx rec_ctx_now(float* saved, int64_t tile, int slot) {
  extern __shared__ __attribute__((aligned(16))) float lds_base[];
  int tid = threadIdx.x;
  asm volatile("" : "+v"(tid));
  const unsigned lane = (unsigned)tid & 63u, j = (unsigned)tid & 31u, hh = ((unsigned)tid >> 5) & 1u;
  const unsigned wave = (unsigned)__builtin_amdgcn_readfirstlane(tid >> 6);
  const unsigned stg = (unsigned)(uintptr_t)AS3(lds_base) + (unsigned)(kBufs * kChunkFloats + kBiasPad) * 4u + wave * 1024u;
  RecCtx c;
  c.recw = stg + ((4u * hh) * 32u + j) * 4u;          // register r -> + (r >> 2) * 4096 + (r & 3) * 128
  c.recr = stg + lane * 16u;                           // unit k -> + k * 4096: feature 8 k + (lane >> 3), samples 4 (lane & 7) ..
  c.ro0 = (unsigned)blk_off(0 + (int)(lane >> 3), (int)(lane & 7u) * 4) * 4u;
  c.ro1 = (unsigned)blk_off(8 + (int)(lane >> 3), (int)(lane & 7u) * 4) * 4u;
  static_assert(blk_off(16 + 3, 12) == blk_off(3, 12) + 512 && blk_off(24 + 6, 20) == blk_off(8 + 6, 20) + 512,
                "units 2 / 3 of a record tile sit 16 rows behind units 0 / 1 with the same swizzle");
  // mask words of slot sl (>= 1) for this lane: kMaskOff + ((sl - 1) * 4 + w) * 64 + lane, relative to the slot's block
  c.mkoff = (unsigned)((kMaskOff + ((slot > 0 ? slot : 1) - 1) * 256 - slot * kBlockFloats) * 4) + lane * 4u;
  const float* base = saved + (tile * 4 + (int64_t)wave) * (int64_t)kSavedGroupFloats + (int64_t)slot * kBlockFloats;
  const uint64_t b = (uint64_t)(uintptr_t)base;
  c.rbase = reinterpret_cast<const float*>((uint64_t)(unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)b) |
                                           ((uint64_t)(unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(b >> 32)) << 32));
  return c;
}
#define TP_REC_INPUTS(r)                                                                                               \
  [recw] "v"(r.recw), [recr] "v"(r.recr), [ro0] "v"(r.ro0), [ro1] "v"(r.ro1), [mkoff] "v"(r.mkoff), [rbase] "s"(r.rbase)

// which recording variant the wide layer `li` runs in the training kernel (it records its SOURCE set): T0 <- L7 = the trunk
// feature (values only), T1 <- T0, T2 <- T1, R1 <- R0, R2 <- R1; R0 re-reads the restored feature: plain
template <class L>
constexpr int rec_kind_of() {
  if constexpr (std::is_same_v<L, int>) return 0;
  else return L::value == T0 ? 2 : (L::value == T1 || L::value == T2 || L::value == R1 || L::value == R2) ? 1 : 0;
}

// WIDE block that also records its SOURCE set; MASK = false: values only (the trunk feature, set Q)
template <bool SRC_Q, bool MASK>
__device__ __forceinline__ void asm_wide_rec(Pipe& p, Frag& f, Guard& amax, const AsmCtx& c, int next_li, const RecCtx& r) {
  TP_RING_LOCALS;
  const float kinv = kInvScale;
  const unsigned mask = 0xFFFFE000u;
  const unsigned nbias = c.bias0 + (unsigned)next_li * 1024u;
  static_assert(SRC_Q || MASK, "the mask-free variant exists for set Q only");
#define TP_WIDE_REC(TXT)                                                                                               \
  asm volatile(TXT : TP_RING(f), TP_RING_STATE, [amax] "+v"(amax.m)                                                    \
               : TP_RING_INPUTS(c), [kinv] "s"(kinv), [mask] "s"(mask), [nbias] "v"(nbias), TP_REC_INPUTS(r)           \
               : TP_ASM_CLOBBERS, TP_ASM_REC_CLOBBERS, "memory", "scc")
  if constexpr (SRC_Q && MASK) TP_WIDE_REC(TP_ASM_WIDE_QP_REC);
  else if constexpr (SRC_Q) TP_WIDE_REC(TP_ASM_WIDE_QP_RECNM);
  else TP_WIDE_REC(TP_ASM_WIDE_PQ_REC);
#undef TP_WIDE_REC
  TP_RING_DONE;
}

// one chunk of KS extra k-steps (staged inputs ks0 .. ks0+KS-1) into set P (DST_P) or Q
template <int KS, bool DST_P>
__device__ __forceinline__ void asm_extra(Pipe& p, Frag& f, const AsmCtx& c, int ks0) {
  TP_RING_LOCALS;
  const unsigned stage = c.stage0 + (unsigned)ks0 * 8192u;
#define TP_EXTRA(TXT)                                                                                                  \
  asm volatile(TXT : TP_RING(f), TP_RING_STATE : TP_RING_INPUTS(c), [stage] "v"(stage)                  \
               : TP_ASM_CLOBBERS, "memory", "scc")
  if constexpr (KS == 1 && DST_P) TP_EXTRA(TP_ASM_EXTRA1_P);
  else if constexpr (KS == 2 && DST_P) TP_EXTRA(TP_ASM_EXTRA2_P);
  else if constexpr (KS == 1) TP_EXTRA(TP_ASM_EXTRA1_Q);
  else TP_EXTRA(TP_ASM_EXTRA2_Q);
#undef TP_EXTRA
  TP_RING_DONE;
}

// single-product arithmetic: KS (1 or 4) extra k-steps of the stage (hi halves only) in one chunk of the f16 stream
template <int KS, bool DST_P>
__device__ __forceinline__ void asm_extra16(Pipe& p, Frag& f, const AsmCtx& c, int ks0) {
  TP_RING_LOCALS;
  const unsigned stage = c.stage0 + (unsigned)ks0 * 8192u;
#define TP_EXTRA16(TXT)                                                                                                \
  asm volatile(TXT : TP_RING(f), TP_RING_STATE : TP_RING_INPUTS(c), [stage] "v"(stage) : TP_ASM_CLOBBERS, "memory", "scc")
  if constexpr (KS == 1 && DST_P) TP_EXTRA16(TP_ASM_EXTRA16_1_P);
  else if constexpr (KS == 4 && DST_P) TP_EXTRA16(TP_ASM_EXTRA16_4_P);
  else if constexpr (KS == 1) TP_EXTRA16(TP_ASM_EXTRA16_1_Q);
  else TP_EXTRA16(TP_ASM_EXTRA16_4_Q);
#undef TP_EXTRA16
  TP_RING_DONE;
}

// narrow output layer over relu(set P) (SRC_P) or relu(set Q): accumulator tile (still scaled by 2^8).  `kinv`: scale of the source
// set (2^-8 for the f16x3 sets; 1 for the unscaled sets of the single-product arithmetic, whose head chunks are f16x3 chunks)
template <bool SRC_P>
__device__ __forceinline__ f32x16 asm_head(Pipe& p, Frag& f, Guard& amax, const AsmCtx& c, float kinv = kInvScale) {
  TP_RING_LOCALS;
  const unsigned mask = 0xFFFFE000u;
  f32x16 acc;
  if constexpr (SRC_P)
    asm volatile(TP_ASM_HEAD_P : TP_RING(f), TP_RING_STATE, [amax] "+v"(amax.m), "=&{v[232:247]}"(acc)
                 : TP_RING_INPUTS(c), [kinv] "s"(kinv), [mask] "s"(mask) : TP_ASM_CLOBBERS, "memory", "scc");
  else
    asm volatile(TP_ASM_HEAD_Q : TP_RING(f), TP_RING_STATE, [amax] "+v"(amax.m), "=&{v[232:247]}"(acc)
                 : TP_RING_INPUTS(c), [kinv] "s"(kinv), [mask] "s"(mask) : TP_ASM_CLOBBERS, "memory", "scc");
  TP_RING_DONE;
  return acc;
}

// the same, also recording the source set (values + ReLU sign words).  Only rows 0..3 of the accumulator tile (registers
// 0..3: rows 0..3 in the lower lane half, 4..7 in the upper) are used by the callers: they come back as four scalars -- as
// a 16-register value the tile was carried, and spilled, through the following sections
struct Head4 { float a0, a1, a2, a3; };
template <bool SRC_P>
__device__ __forceinline__ Head4 asm_head_rec(Pipe& p, Frag& f, Guard& amax, const AsmCtx& c, const RecCtx& r) {
  TP_RING_LOCALS;
  const float kinv = kInvScale;
  const unsigned mask = 0xFFFFE000u;
  Head4 h;
#define TP_HEAD_REC(TXT)                                                                                               \
  asm volatile(TXT : TP_RING(f), TP_RING_STATE, [amax] "+v"(amax.m), "=&{v232}"(h.a0), "=&{v233}"(h.a1),               \
                     "=&{v234}"(h.a2), "=&{v235}"(h.a3)                                                                \
               : TP_RING_INPUTS(c), [kinv] "s"(kinv), [mask] "s"(mask), TP_REC_INPUTS(r)                               \
               : TP_ASM_CLOBBERS, TP_ASM_REC_CLOBBERS, "v236", "v237", "v238", "v239", "v240", "v241", "v242", "v243", \
                 "v244", "v245", "v246", "v247", "memory", "scc")
  if constexpr (SRC_P) TP_HEAD_REC(TP_ASM_HEAD_P_REC);
  else TP_HEAD_REC(TP_ASM_HEAD_Q_REC);
#undef TP_HEAD_REC
  TP_RING_DONE;
  return h;
}

// fp32 vector-ALU head of the ray-bias kernel (gen_head_valu): WHICH = 0 sigma (set P, 1 row), 1 transient (set P, 5 rows), 2 rgb
// (set Q, 3 rows), weights from the LDS table (kernel start).  Outside the ring protocol: no chunk is consumed; the fragment ring's
// registers are used as scratch and re-read from the current chunk's slot at the end.  Every lane gets every row's sum (still scaled
// by 2^8)
struct Head5 { float r0, r1, r2, r3, r4; };
template <int WHICH>
__device__ __forceinline__ Head5 asm_head_valu(const Pipe& p, Frag& f, const AsmCtx& c) {
  int tid = threadIdx.x;
  asm volatile("" : "+v"(tid));
  const unsigned hw = c.stage0 - (unsigned)tid * 16u + (((unsigned)tid >> 5) & 1u) * 16u;   // stage base + 16 h
  const int buf = __builtin_amdgcn_readfirstlane(p.buf);
  int t0;
  Head5 h;
#define TP_HEADV(TXT)                                                                                                  \
  asm volatile(TXT : TP_RING(f), [t0] "=&s"(t0), "=&{v232}"(h.r0), "=&{v233}"(h.r1), "=&{v234}"(h.r2), "=&{v235}"(h.r3), \
                     "=&{v236}"(h.r4)                                                                                  \
               : [hw] "v"(hw), [lane16] "v"(c.lane16), [buf] "s"(buf)                                                  \
               : TP_ASM_CLOBBERS, "v231", "v237", "v238", "v239", "v240", "v241", "v242", "v243", "v244", "v245", "v246", "v247", \
                 "memory", "scc")
  if constexpr (WHICH == 0) TP_HEADV(TP_ASM_HEADV_P1);
  else if constexpr (WHICH == 1) TP_HEADV(TP_ASM_HEADV_P5);
  else TP_HEADV(TP_ASM_HEADV_Q3);
#undef TP_HEADV
  return h;
}

// seed set P (DST_P) or Q with the bias block of wide layer li (bias * 2^8 in LDS)
template <bool DST_P>
__device__ __forceinline__ void asm_init(const AsmCtx& c, int li) {
  const unsigned bias = c.bias0 + (unsigned)li * 1024u;
  if constexpr (DST_P) asm volatile(TP_ASM_INIT_P :: [bias] "v"(bias) : TP_ASM_CLOBBERS, "memory");
  else asm volatile(TP_ASM_INIT_Q :: [bias] "v"(bias) : TP_ASM_CLOBBERS, "memory");
}

struct Params {
  const float* packed;
  const float* center; const float* ray; const float* depth;
  const float* points; const float* ray_unit;
  const float* lat_trans; const float* lat_light;
  int B, R, N;
  int64_t n_samples, n_tiles;
  float* rgb; float* density; float* uncert; float* saved; float* workspace; int* status;
  const float* density_noise;      // optional: added to the static density's pre-activation (nerf.density_noise_reg, train mode)
  unsigned int* act_max;
  const float* ray_bias;     // RB kernels: [B][2][256] per-image part, then [B*R][256] per-ray accumulator seeds of R0 (rb_*_kernel below)
};

// stage one "extra input" value as hi/lo halves: slot = 16 ks + 8 h + j of this lane
__device__ __forceinline__ void stage(_Float16* st, int tid, int ks, int j, float v) {
  const _Float16 hi = (_Float16)v;
  st[((ks * 2 + 0) * kThreads + tid) * 8 + j] = hi;
  st[((ks * 2 + 1) * kThreads + tid) * 8 + j] = (_Float16)(v - (float)hi);
}

// the same for an arbitrary slot of this SAMPLE (either lane of the sample's lane pair may own it): tid_lo = tid & ~32
__device__ __forceinline__ void stage_slot(_Float16* st, int tid_lo, int slot, float v) {
  const int ks = slot >> 4, owner = tid_lo | ((slot & 8) << 2), jj = slot & 7;
  const _Float16 hi = (_Float16)v;
  st[((ks * 2 + 0) * kThreads + owner) * 8 + jj] = hi;
  st[((ks * 2 + 1) * kThreads + owner) * 8 + jj] = (_Float16)(v - (float)hi);
}

// Thread coordinates are RE-DERIVED from the hardware id at the top of every section of the tile loop (the empty volatile asm
// keeps the derivations apart): carried through the asm blocks they lived in scratch memory, like the block context above.
#define TP_THREAD_IDS                                                                                                  \
  int tid = threadIdx.x;                                                                                               \
  asm volatile("" : "+v"(tid));                                                                                        \
  const int lane = tid & 63, j = tid & 31, hh = (tid >> 5) & 1;                                                        \
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);                                                           \
  float* save = reinterpret_cast<float*>(st + kStageHalves) + tid;                                                     \
  (void)lane; (void)j; (void)hh; (void)wave; (void)save

// RB ("ray bias", evaluation only): the stream of chunk_desc_rb (mlp_layout.h).  Every tile lies inside one ray (N % 128 == 0); the
// accumulators of R0 / T0 are seeded with the per-ray / per-image bias the pre-kernels below left in P.ray_bias, nothing is staged for
// T0 and R0, and R0's only extra k-step re-reads x from k-step 3 of the encoding stage.
// F16 (TP_MLP_F16, inference only): the single-product arithmetic on the f16 stream (mlp_layout.h) -- the 256-wide layers and their
// extra inputs run the WIDE16 / EXTRA16 blocks, the sets are NOT scaled by 2^8 (unscaled biases, weights and ray-bias seeds), the narrow
// output layers are the f16x3 ones (HEAD over an unscaled set: kinv = 1; the fp32 VALU head of the ray-bias form with its table
// scaled by 2^8), so the head epilogue is unchanged.  Everything else -- schedule, ring, staging, stash, status words -- is shared.
template <bool SAVE, bool RB = false, bool F16 = false>
__global__ __launch_bounds__(kThreads, 1) void mlp_fwd_f16x3_kernel(Params P) {
  static_assert(!(SAVE && RB), "the ray-bias stream has no recording variant");
  static_assert(!(SAVE && F16), "the single-product arithmetic is inference only");
  constexpr int NCH = F16 ? (RB ? kNumChunks16RB : kNumChunks16) : (RB ? kNumChunksRB : kNumChunks);
  constexpr int BIAS_NCH = RB ? kNumChunksRB : kNumChunks;      // (the f16 streams keep their bias / aux blocks where f16x3 does)
  constexpr float kSetScale = F16 ? 1.0f : (float)(1 << kF16WeightShift);    // accumulator sets hold  scale * (W x + b)
#define TP_CTX asm_ctx_now(P.packed, NCH)
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  float* bias_lds = lds + kBufs * kChunkFloats;
  _Float16* st = reinterpret_cast<_Float16*>(bias_lds + kBiasPad);     // then the lane-private save area: save[k * kThreads], k < 8

  Pipe p;
  p.stream = P.packed; p.lds = lds; p.chunk = 0; p.buf = 0; p.wave = __builtin_amdgcn_readfirstlane(wave); p.lane = lane;
  // wide-layer biases are kept pre-scaled by 2^8 (exact): they seed the accumulators of the scaled products
  for (int i = tid; i < kBiasFloats; i += kThreads)
    bias_lds[i] = P.packed[(size_t)BIAS_NCH * kChunkFloats + i] * (i < kHeadBiasOff ? kSetScale : 1.0f);
  if constexpr (RB) {
    // the nine rows of the narrow output layers (fp32, lane-read order) into the parts of the input stage / save area this kernel
    // does not use: k-step 4 of the stage and slot 6 of the save area (gen_wide_asm.py: HEADTAB_*)
    constexpr int kHeadTabOff[kRbHeadRows] = TP_HEADTAB_OFFSETS;
    const float* tab = P.packed + kRbAuxOff + kRbAuxHeads;
    for (int i = tid; i < kRbHeadRows * 256; i += kThreads)
      *reinterpret_cast<float*>(reinterpret_cast<char*>(st) + kHeadTabOff[i >> 8] + (i & 255) * 4) =
          tab[i] * ((float)(1 << kF16WeightShift) / kSetScale);      // (F16: 2^8, exact, so the head sums come back scaled as in f16x3)
  }
  dma_chunk(p, 0, 0);
  dma_chunk(p, 1, 1);
  __syncthreads();
  Frag frag;
  frag_prime(p, frag);
  // (round 1 staggered the start phases of the persistent workgroups by up to 256 us so that they would not park their
  // trunk features at the same instant; with the feature held in registers the stagger buys nothing on a full image and
  // cost 9 % of a B=4 training step, whose recording forward is only two tiles per CU)
#ifdef TP_TRACE
  const long long tr_start = tick();
#endif
  asm_init<true>(TP_CTX, L0);        // set P starts as L0's bias; from then on every wide layer re-seeds its source set

  for (int64_t tile = blockIdx.x; tile < P.n_tiles; tile += gridDim.x) {
    TR_BEGIN(pro);
    TP_THREAD_IDS;
    const int64_t s_raw = tile * 128 + wave * 32 + j;
    const bool live = s_raw < P.n_samples;
    const int64_t s = live ? s_raw : 0;            // (dead lanes recompute sample 0: any valid index; a literal needs no register)
    const int64_t q = s / P.N;
    const int b = (int)(q / P.R);
    // Everything the later staging steps need of this sample goes to a lane-private LDS area, not through registers:
    // between the asm blocks the compiler owns few VGPRs (the blocks' working set, the fragment ring and, from L7 to
    // R0, the trunk feature are fixed), and values carried across them would end up in scratch memory
    {
      float x0, x1, x2, vu0, vu1, vu2;
      if (P.center != nullptr) {
        const float z = P.depth[s];
        const float d0 = P.ray[3 * q + 0], d1 = P.ray[3 * q + 1], d2 = P.ray[3 * q + 2];
        x0 = tp::add_rn(P.center[3 * q + 0], tp::mul_rn(d0, z));
        x1 = tp::add_rn(P.center[3 * q + 1], tp::mul_rn(d1, z));
        x2 = tp::add_rn(P.center[3 * q + 2], tp::mul_rn(d2, z));
        float nrm = tp::add_rn(0.f, tp::mul_rn(d0, d0));
        nrm = tp::add_rn(nrm, tp::mul_rn(d1, d1));
        nrm = tp::add_rn(nrm, tp::mul_rn(d2, d2));
        const float den = fmaxf(sqrtf(nrm), 1e-12f);
        vu0 = tp::div_rn(d0, den); vu1 = tp::div_rn(d1, den); vu2 = tp::div_rn(d2, den);
      } else {
        x0 = P.points[3 * s + 0]; x1 = P.points[3 * s + 1]; x2 = P.points[3 * s + 2];
        vu0 = P.ray_unit[3 * s + 0]; vu1 = P.ray_unit[3 * s + 1]; vu2 = P.ray_unit[3 * s + 2];
      }
      save[0 * kThreads] = x0; save[1 * kThreads] = x1; save[2 * kThreads] = x2;
      if constexpr (!RB) {
        save[3 * kThreads] = vu0; save[4 * kThreads] = vu1; save[5 * kThreads] = vu2;
        save[6 * kThreads] = __int_as_float(b);
      } else {
        // this tile's accumulator seeds of R0 (per ray) and T0 (per image), already scaled by 2^8 and in bias-block order: one float
        // per thread each.  The blocks that read them (T2 re-seeds set Q for R0, L7 re-seeds set P for T0) are many barriers away;
        // the previous tile's reads of these two blocks lie before its last barriers.
        const int64_t qt = (tile * 128) / P.N;                 // (wave-uniform: the tile's ray)
        // (the pre-kernels scale by 2^8; F16 sets are unscaled: * 2^-8, exact)
        bias_lds[R0 * 256 + tid] = P.ray_bias[(size_t)P.B * 512 + (size_t)qt * 256 + tid] * (kSetScale * kInvScale);
        bias_lds[T0 * 256 + tid] = P.ray_bias[(size_t)(qt / P.R) * 512 + tid] * (kSetScale * kInvScale);
      }
    }
    asm_init<false>(TP_CTX, L1);       // set Q for L1 (set P was re-seeded for L0 by the previous tile's last layer)
    TR_END(4, pro);
    // The two accumulator sets: even layers read Q and accumulate into P, odd layers the reverse (the layer loop is
    // unrolled by two, so both roles are fixed registers).  A set holds raw accumulators, bias included (seeded with
    // bias * 2^8); the next layer's B operands are produced from it inside the asm blocks.
    f32x16 SF[8];               // the trunk feature (L7's accumulators), held in v[32:159] from L7 to R0
    Guard amax;
    float sig_s, rgb_s[3], ta0, ta1, ta2, ta3;          // (no initial values: they would be live through every block)
    const float* hbias = bias_lds + kHeadBiasOff;          // [b7[0], T3 bias 0..4, R3 bias 0..2]

    // a narrow output layer; which == 0: sigma (reads L6 = set P), 1: transient head (reads T2 = set P), 2: static
    // rgb (reads R2 = set Q).  The transient head's result comes back while the trunk feature still occupies 128 VGPRs:
    // its non-linearities run after the feature has been restored into set P (`after`)
    const auto head = [&](auto which_tag, auto after) {
      constexpr int which = decltype(which_tag)::value;
      TR_BEGIN(h);
      // training: the heads over T2 (set P) / R2 (set Q) also write those layers' activation records
      float a0, a1, a2, a3;
      if constexpr (SAVE && which != 0) {
        Head4 h4;
        if constexpr (which == 2) h4 = asm_head_rec<false>(p, frag, amax, TP_CTX, rec_ctx_now(P.saved, tile, SV_R2));
        else h4 = asm_head_rec<true>(p, frag, amax, TP_CTX, rec_ctx_now(P.saved, tile, SV_T2));
        a0 = h4.a0; a1 = h4.a1; a2 = h4.a2; a3 = h4.a3;
        TR_END(7, h);
      } else if constexpr (RB) {
        // ray-bias stream: the heads are fp32 dot products on the vector ALU; every lane gets every row (the matrix-core form
        // leaves rows 0..3 in the lower lane half and row 4 in register 0 of the upper one: same hand-over below)
        const Head5 h5 = asm_head_valu<which>(p, frag, TP_CTX);
        TR_END(7, h);
        TP_THREAD_IDS;
        a0 = (which == 1 && hh) ? h5.r4 : h5.r0; a1 = h5.r1; a2 = h5.r2; a3 = h5.r3;
      } else {
        f32x16 a;
        if constexpr (which == 2) a = asm_head<false>(p, frag, amax, TP_CTX, 1.0f / kSetScale);
        else a = asm_head<true>(p, frag, amax, TP_CTX, 1.0f / kSetScale);
        TR_END(7, h);
        a0 = a[0]; a1 = a[1]; a2 = a[2]; a3 = a[3];
      }
      after();
      if (which == 0) {
        float dn = 0.0f;
        if (P.density_noise != nullptr) {          // (uniform branch; the sample index is re-derived here, not carried through the tile)
          TP_THREAD_IDS;
          int64_t sn = tile * 128 + wave * 32 + j;
          if (sn >= P.n_samples) sn = P.n_samples - 1;
          dn = P.density_noise[sn];
        }
        sig_s = softplus(fmaf(a0, kInvScale, hbias[0]) + dn);
      } else if (which == 1) {
        // raw accumulators only: the non-linearities run at the end of the R0 staging section (no asm block in between),
        // whose results go to the lane-private LDS area -- held in registers until the output section they crossed R0..R2
        // in scratch memory, and stored early as 4-byte pieces they doubled the write traffic
        ta0 = a0; ta1 = a1; ta2 = a2; ta3 = a3;
      } else {
        rgb_s[0] = sigmoid(fmaf(a0, kInvScale, hbias[6])); rgb_s[1] = sigmoid(fmaf(a1, kInvScale, hbias[7]));
        rgb_s[2] = sigmoid(fmaf(a2, kInvScale, hbias[8]));
      }
    };

    // one wide layer: EVEN layers read set Q and accumulate into set P, odd layers the reverse
    // `li_arg`: the wide-layer index as a run-time int (the rolled trunk loop) or as an integral_constant (training: the six
    // head layers are unrolled, so that every asm statement of a recording block sits at a call site of its own -- with the
    // recording and the plain variant behind a run-time branch on `li` at ONE site the register allocator spilled a
    // 16-register tile of the stashed trunk feature around it)
    const auto layer = [&](auto even_tag, auto li_arg) {
      constexpr bool EVEN = decltype(even_tag)::value;
      const int li = li_arg;
      constexpr int REC = SAVE ? rec_kind_of<decltype(li_arg)>() : 0;      // 0 plain, 1 values + sign words, 2 values only
      if (!EVEN && li == L7) head(std::integral_constant<int, 0>{}, [] {});                              // sigma: reads set P (L6)
      if (!EVEN && li == R0)                                               // transient head: reads set P (T2); then the
        head(std::integral_constant<int, 1>{}, [&] {                                                      // trunk feature comes back into that set
          TR_BEGIN(rl);
          asm_restore_p(SF);
          TR_END(10, rl);
        });

      if (li != L0) {
        TR_BEGIN(w);
        const int next_li = li + 1 == kNumWide ? 0 : li + 1;
        // training: a wide layer whose SOURCE set is a recorded activation writes that record while it converts it
        // (T0 <- L7 = trunk feature, values only; T1 <- T0; T2 <- T1; R1 <- R0; R2 <- R1.  R0 re-reads the restored feature)
        if constexpr (REC == 2) asm_wide_rec<true, false>(p, frag, amax, TP_CTX, next_li, rec_ctx_now(P.saved, tile, SV_FEAT));
        else if constexpr (REC == 1) asm_wide_rec<EVEN, true>(p, frag, amax, TP_CTX, next_li, rec_ctx_now(P.saved, tile, li - 1 - L7));
        else if constexpr (F16) asm_wide16<EVEN>(p, frag, amax, TP_CTX, next_li);
        else asm_wide<EVEN>(p, frag, amax, TP_CTX, next_li);
        TR_END(3, w);
      }

      if (EVEN && (li == L0 || li == L4)) {
        // [PE(x) | x | pad] in natural column order; this lane stages slots 16 ks + 8 h + jj.  Staged once per tile:
        // the skip connection (L4) re-reads what L0 staged, nothing overwrites it before T0
        TR_BEGIN(pe);
        // 30 (coordinate, octave) pairs, 15 per lane of the sample's lane pair: one range reduction yields the sin AND
        // the cos entry (slots 20 c + l and 20 c + 10 + l, whichever lane's operand registers they belong to)
        if (li == L0) {
          TP_THREAD_IDS;
          const float x0 = save[0 * kThreads], x1 = save[1 * kThreads], x2 = save[2 * kThreads];
          // ONE fp64 range reduction per coordinate, then the ten octaves by angle doubling (tp::sincos_f64: the argument of octave
          // l is exactly 2^l * fl32(x pi_f32)).  Lane hh of the sample's lane pair runs the chain of coordinate 2 hh and stages its
          // sin AND cos entries (slots 20 c + l, 20 c + 10 + l); both lanes run the chain of coordinate 1, lane 0 stages its sin
          // entries, lane 1 its cos entries: 30 slots per lane as before, two independent chains in flight.
          const int ca = 2 * hh;
          tp::SinCos64 ea = tp::sincos_f64(tp::mul_rn(hh ? x2 : x0, 3.14159274101257324f));
          tp::SinCos64 eb = tp::sincos_f64(tp::mul_rn(x1, 3.14159274101257324f));
#pragma unroll
          for (int l = 0; l < 10; ++l) {
            stage_slot(st, tid & ~32, 20 * ca + l, (float)ea.s);
            stage_slot(st, tid & ~32, 20 * ca + 10 + l, (float)ea.c);
            stage_slot(st, tid & ~32, 20 + 10 * hh + l, (float)(hh ? eb.c : eb.s));
            if (l < 9) { tp::sincos_double(ea); tp::sincos_double(eb); }
          }
          if (hh) {
            stage(st, tid, 3, 4, x0); stage(st, tid, 3, 5, x1); stage(st, tid, 3, 6, x2); stage(st, tid, 3, 7, 0.0f);
          }
        }
        TR_END(5, pe);
        TR_BEGIN(w);
        if constexpr (F16) {
          asm_extra16<4, true>(p, frag, TP_CTX, 0);
        } else {
          asm_extra<2, true>(p, frag, TP_CTX, 0);
          asm_extra<2, true>(p, frag, TP_CTX, 2);
        }
        TR_END(3, w);
      } else if (RB && EVEN && li == T0) {
        // (the transient code is in the layer's per-image bias)
      } else if (RB && !EVEN && li == R0) {
        // the transient head's non-linearities (see the staging section of the plain kernel below); x has been consumed by L0
        TR_BEGIN(r0s);
        TP_THREAD_IDS;
        if (hh == 0) {
          save[0 * kThreads] = sigmoid(fmaf(ta0, kInvScale, hbias[1]));
          save[1 * kThreads] = sigmoid(fmaf(ta1, kInvScale, hbias[2]));
          save[2 * kThreads] = sigmoid(fmaf(ta2, kInvScale, hbias[3]));
          save[3 * kThreads] = softplus(fmaf(ta3, kInvScale, hbias[4]));
        } else {
          save[0 * kThreads] = softplus(fmaf(ta0, kInvScale, hbias[5]));
        }
        TR_END(6, r0s);
        TR_BEGIN(w);
        if constexpr (F16) asm_extra16<1, false>(p, frag, TP_CTX, 3);
        else asm_extra<1, false>(p, frag, TP_CTX, 3);          // [PE slots 48..59 (zero weights) | x | 0] as staged for L0
        TR_END(3, w);
      } else if (EVEN && li == T0) {
        TR_BEGIN(t0s);
        TP_THREAD_IDS;
        const int bt = __float_as_int(save[6 * kThreads]);
#pragma unroll
        for (int jj = 0; jj < 8; ++jj) stage(st, tid, 0, jj, P.lat_trans[bt * 16 + 8 * hh + jj]);
        TR_END(13, t0s);
        TR_BEGIN(w);
        if constexpr (F16) asm_extra16<1, true>(p, frag, TP_CTX, 0);
        else asm_extra<1, true>(p, frag, TP_CTX, 0);
        TR_END(3, w);
      } else if (!EVEN && li == R0) {
        // [ray_unit | PE(ray_unit) | x | light] in natural column order, 78 of 80 slots
        TR_BEGIN(r0s);
        TP_THREAD_IDS;
        // slots 0..31: ray_unit (0..2), PE(ray_unit) (3 + 8 c + 4 sc + l: 12 sin/cos pairs, 6 per lane), x (27..29),
        // the first two latent entries (30, 31).  Training: slots 0..29 (mlp_rgb.0 input columns 256..285) also go
        // to the activation record as fp32 for the weight gradient
        float* sx = SAVE ? P.saved + (tile * 4 + wave) * (int64_t)kSavedGroupFloats + SV_EX * kBlockFloats : nullptr;
        const float x0 = save[0 * kThreads], x1 = save[1 * kThreads], x2 = save[2 * kThreads];
        const float vu0 = save[3 * kThreads], vu1 = save[4 * kThreads], vu2 = save[5 * kThreads];
        const int br = __float_as_int(save[6 * kThreads]);
        // the view encoding (4 octaves) the same way: chain of coordinate 2 hh (sin and cos), chain of coordinate 1 (lane 0 its sin
        // entries, lane 1 its cos entries); slot 3 + 8 c + l = sin, + 4 = cos
        {
          const int ca = 2 * hh;
          tp::SinCos64 ea = tp::sincos_f64(tp::mul_rn(hh ? vu2 : vu0, 3.14159274101257324f));
          tp::SinCos64 eb = tp::sincos_f64(tp::mul_rn(vu1, 3.14159274101257324f));
#pragma unroll
          for (int l = 0; l < 4; ++l) {
            const float sa = (float)ea.s, cav = (float)ea.c, vb = (float)(hh ? eb.c : eb.s);
            const int s0 = 3 + 8 * ca + l, s1 = 3 + 8 + 4 * hh + l;
            stage_slot(st, tid & ~32, s0, sa);
            stage_slot(st, tid & ~32, s0 + 4, cav);
            stage_slot(st, tid & ~32, s1, vb);
            if (SAVE && live) { sx[blk_off(s0, j)] = sa; sx[blk_off(s0 + 4, j)] = cav; sx[blk_off(s1, j)] = vb; }
            if (l < 3) { tp::sincos_double(ea); tp::sincos_double(eb); }
          }
        }
        if (hh == 0) {
          stage(st, tid, 0, 0, vu0); stage(st, tid, 0, 1, vu1); stage(st, tid, 0, 2, vu2);
          if (SAVE && live) { sx[blk_off(0, j)] = vu0; sx[blk_off(1, j)] = vu1; sx[blk_off(2, j)] = vu2; }
        } else {
          stage(st, tid, 1, 3, x0); stage(st, tid, 1, 4, x1); stage(st, tid, 1, 5, x2);
          stage(st, tid, 1, 6, P.lat_light[br * 48 + 0]); stage(st, tid, 1, 7, P.lat_light[br * 48 + 1]);
          if (SAVE && live) { sx[blk_off(27, j)] = x0; sx[blk_off(28, j)] = x1; sx[blk_off(29, j)] = x2; }
        }
        // k-steps 2..4 are latent-code slots only: 8 loads at a time (one latency per k-step), one 16-byte store per
        // (k-step, hi/lo)
#pragma unroll
        for (int ks = 2; ks < 5; ++ks) {
          float lv[8];
#pragma unroll
          for (int jj = 0; jj < 8; ++jj) {
            const int slot = 16 * ks + 8 * hh + jj;
            lv[jj] = slot < 78 ? P.lat_light[br * 48 + slot - 30] : 0.0f;
          }
          half8 hi8, lo8;
#pragma unroll
          for (int jj = 0; jj < 8; ++jj) {
            hi8[jj] = (_Float16)lv[jj];
            lo8[jj] = (_Float16)(lv[jj] - (float)hi8[jj]);
          }
          *reinterpret_cast<half8*>(st + ((ks * 2 + 0) * kThreads + tid) * 8) = hi8;
          *reinterpret_cast<half8*>(st + ((ks * 2 + 1) * kThreads + tid) * 8) = lo8;
        }
        // the transient head's non-linearities (its raw accumulators came through the staging code above in registers);
        // x / view direction / image index have been consumed: their LDS slots carry the results to the output section
        if (hh == 0) {
          save[0 * kThreads] = sigmoid(fmaf(ta0, kInvScale, hbias[1]));
          save[1 * kThreads] = sigmoid(fmaf(ta1, kInvScale, hbias[2]));
          save[2 * kThreads] = sigmoid(fmaf(ta2, kInvScale, hbias[3]));
          save[3 * kThreads] = softplus(fmaf(ta3, kInvScale, hbias[4]));
        } else {
          save[0 * kThreads] = softplus(fmaf(ta0, kInvScale, hbias[5]));       // row 4 = register 0 of the upper lane half
        }
        TR_END(6, r0s);
        TR_BEGIN(w);
        if constexpr (F16) {
          asm_extra16<4, false>(p, frag, TP_CTX, 0);
          asm_extra16<1, false>(p, frag, TP_CTX, 4);
        } else {
          asm_extra<2, false>(p, frag, TP_CTX, 0);
          asm_extra<2, false>(p, frag, TP_CTX, 2);
          asm_extra<1, false>(p, frag, TP_CTX, 4);
        }
        TR_END(3, w);
      }

      if (!EVEN && li == L7) {
        // keep the trunk feature (raw accumulators of L7, set Q) for R0: T1 overwrites set Q
        TR_BEGIN(vc);
        asm_stash_q(SF);
        TR_END(9, vc);
      }
    };

    if constexpr (SAVE) {
#pragma nounroll
      for (int pr = 0; pr < 4; ++pr) {                 // L0 .. L7
        layer(std::true_type{}, 2 * pr);
        layer(std::false_type{}, 2 * pr + 1);
      }
      layer(std::true_type{}, std::integral_constant<int, T0>{});
      layer(std::false_type{}, std::integral_constant<int, T1>{});
      layer(std::true_type{}, std::integral_constant<int, T2>{});
      layer(std::false_type{}, std::integral_constant<int, R0>{});
      layer(std::true_type{}, std::integral_constant<int, R1>{});
      layer(std::false_type{}, std::integral_constant<int, R2>{});
    } else {
#pragma nounroll
      for (int pr = 0; pr < kNumWide / 2; ++pr) {
        layer(std::true_type{}, 2 * pr);
        layer(std::false_type{}, 2 * pr + 1);
      }
    }
    head(std::integral_constant<int, 2>{}, [] {});

    TR_BEGIN(o);
    {
      // output section: sample index recomputed here (and hidden from the optimiser: addresses formed at the top of the
      // tile would have to live through every block, i.e. in scratch memory)
      TP_THREAD_IDS;
      int64_t so = tile * 128 + wave * 32 + j;
      asm volatile("" : "+v"(so));
      if (so < P.n_samples) {
        if (hh == 0) {
          // streaming stores (the outputs are never read by this kernel); the transient head's values come back from LDS
          float* o = P.rgb + so * 6;
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            __builtin_nontemporal_store(rgb_s[c], o + 2 * c);
            __builtin_nontemporal_store(save[c * kThreads], o + 2 * c + 1);
          }
          __builtin_nontemporal_store(sig_s, P.density + so * 2);
          __builtin_nontemporal_store(save[3 * kThreads], P.density + so * 2 + 1);
        } else {
          __builtin_nontemporal_store(save[0 * kThreads], P.uncert + so);
        }
      }
    }
    const float tile_max = fmaxf((float)amax.m[0], (float)amax.m[1]);
    if (P.status != nullptr && !(tile_max < 6.0e4f)) atomicOr(P.status, 1);
    if (P.act_max != nullptr) {
      // largest hidden activation of the tile (non-negative floats order like their bit patterns): one atomic per wave.
      // The lane id comes from a volatile asm (a plain __lane_id() / __shfl_xor is hoisted out of the tile loop and then
      // lives through every block, i.e. in scratch memory); the butterfly uses ds_bpermute with that id
      int lid;
      asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(lid));
      float wmax = tile_max;
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1)
        wmax = fmaxf(wmax, __int_as_float(__builtin_amdgcn_ds_bpermute((lid ^ off) << 2, __float_as_int(wmax))));
      if (lid == 0 && wmax == wmax) atomicMax(P.act_max, __float_as_uint(wmax));
    }
    TR_END(11, o);
  }
#ifdef TP_TRACE
  if (lane == 0 && blockIdx.x == 100 && wave == 1 && P.n_tiles > 1000) {
    const long long tot = tick() - tr_start;
    printf("trace total %lld | dma %lld vm %lld bar %lld wide %lld | pro %lld pe %lld r0 %lld heads %lld | init %lld park %lld reload %lld out %lld | gen0 %lld t0stage %lld\n",
           tot, p.tr[0], p.tr[1], p.tr[2], p.tr[3], p.tr[4], p.tr[5], p.tr[6], p.tr[7], p.tr[8], p.tr[9], p.tr[10], p.tr[11], p.tr[12], p.tr[13]);
  }
#endif
}
#undef TP_CTX

// ---- pre-kernels of the ray-bias variant (mlp_layout.h): accumulator seeds of T0 per image and of R0 per ray, fp32 FMA chains
// over the transposed weight columns in the aux block of the stream, written in bias-block order (thread e <-> (h, t, r) of
// bias_index, feature feat_of(t, r, h)) and scaled by 2^8 like the bias block in LDS.
//   out[b][0][e] = 2^8 (b_T0[f] + sum_c W_T0[f][256 + c] trans[b][c])        (mlp_trans.0, reference layers/...light.py:127-131)
//   out[b][1][e] =      b_R0[f] + sum_c W_R0[f][286 + c] light[b][c]          (unscaled: the per-image part of the ray kernel's sum)
__global__ __launch_bounds__(256) void rb_image_bias_kernel(const float* __restrict__ packed, const float* __restrict__ lat_trans,
                                                            const float* __restrict__ lat_light, float* __restrict__ out) {
  const int b = blockIdx.x, e = threadIdx.x;
  const int h = e >> 7, t = (e >> 4) & 7, r = e & 15, f = feat_of(t, r, h);
  const float* bias = packed + (size_t)kNumChunksRB * kChunkFloats;
  const float* aux = packed + kRbAuxOff;
  float at = bias[bias_index(T0, h, t, r)];
#pragma unroll
  for (int c = 0; c < 16; ++c) at = fmaf(aux[kRbAuxTrans + c * 256 + f], lat_trans[b * 16 + c], at);
  float al = bias[bias_index(R0, h, t, r)];
#pragma unroll 8
  for (int c = 0; c < 48; ++c) al = fmaf(aux[kRbAuxLight + c * 256 + f], lat_light[b * 48 + c], al);
  out[(size_t)b * 512 + e] = at * (float)(1 << kF16WeightShift);
  out[(size_t)b * 512 + 256 + e] = al;
}

//   out[q][e] = 2^8 (img[b][1][e] + sum_c W_R0[f][256 + c] enc_q[c]),   enc_q = [ray_unit(3) | PE(ray_unit): 3 + 8 c + 4 sc + l]
// with ray_unit and its encoding formed exactly as the plain kernel stages them (same normalisation, same fp64 reduction + angle
// doubling), reference layers/...light.py:104-110.  One workgroup: kRbRays rays, thread e = one output feature.
constexpr int kRbRays = 32;
__global__ __launch_bounds__(256) void rb_ray_bias_kernel(const float* __restrict__ packed, const float* __restrict__ ray, int R,
                                                          int64_t n_rays, const float* __restrict__ img, float* __restrict__ out) {
  __shared__ float enc[kRbRays][28];
  const int e = threadIdx.x;
  const int64_t q0 = (int64_t)blockIdx.x * kRbRays;
  if (e < kRbRays * 3) {
    // thread (ray i, coordinate c): the unit direction's component and its four octaves
    const int i = e / 3, c = e - 3 * i;
    const int64_t q = q0 + i < n_rays ? q0 + i : n_rays - 1;
    const float d0 = ray[3 * q + 0], d1 = ray[3 * q + 1], d2 = ray[3 * q + 2];
    float nrm = tp::add_rn(0.f, tp::mul_rn(d0, d0));
    nrm = tp::add_rn(nrm, tp::mul_rn(d1, d1));
    nrm = tp::add_rn(nrm, tp::mul_rn(d2, d2));
    const float den = fmaxf(sqrtf(nrm), 1e-12f);
    const float vu = tp::div_rn(c == 0 ? d0 : (c == 1 ? d1 : d2), den);
    enc[i][c] = vu;
    tp::SinCos64 a = tp::sincos_f64(tp::mul_rn(vu, 3.14159274101257324f));
#pragma unroll
    for (int l = 0; l < 4; ++l) {
      enc[i][3 + 8 * c + l] = (float)a.s;
      enc[i][3 + 8 * c + 4 + l] = (float)a.c;
      if (l < 3) tp::sincos_double(a);
    }
  }
  const int h = e >> 7, t = (e >> 4) & 7, r = e & 15, f = feat_of(t, r, h);
  const float* aux = packed + kRbAuxOff + kRbAuxView;
  float w[27];
#pragma unroll
  for (int c = 0; c < 27; ++c) w[c] = aux[c * 256 + f];
  __syncthreads();
  for (int i = 0; i < kRbRays; ++i) {
    const int64_t q = q0 + i;
    if (q >= n_rays) break;
    float a = img[(size_t)(q / R) * 512 + 256 + e];
#pragma unroll
    for (int c = 0; c < 27; ++c) a = fmaf(w[c], enc[i][c], a);
    out[(size_t)q * 256 + e] = a * (float)(1 << kF16WeightShift);
  }
}

// =====================================================================================================================
// Split-fp16 dgrad (backward of the two heads wrt their hidden activations): the structure of mlp_dgrad_kernel
// (mlp_bwd.hip) -- dh = W^T dz layer by layer, ReLU gates from the recorded sign bits, every dz block written to the
// gradient record for the weight-gradient GEMM -- on the f16 matrix cores with the machinery of the forward above:
// transposed f16x3 weight stream (34 chunks, chunkT16_src), two accumulator sets in ping-pong, operands converted in
// the MFMA issue gaps.  Gradients are tiny (1e-9 .. 1e-2), far below the fp16 normal range, so each sample's chain is
// scaled by a power of two chosen from its own output-layer derivatives (both lanes of a sample compute the same
// factor): exact, linear through the masked chain, undone when a dz block is stored.
// =====================================================================================================================
struct WT { const float* w[16]; };

__global__ void packT16_kernel(WT w, _Float16* __restrict__ out) {
  const int64_t n = (int64_t)kNumChunksT * kChunkHalves;
  const float scale = (float)(1 << kF16WeightShift);
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x) {
    int part, mat, o, f;
    chunkT16_src((int)(e / kChunkHalves), (int)(e % kChunkHalves), part, mat, o, f);
    const float v = o < 0 ? 0.0f : w.w[mat][(int64_t)o * 256 + f] * scale;
    const _Float16 hi = (_Float16)v;
    out[e] = part == 0 ? hi : (_Float16)(v - (float)hi);
  }
}

struct DgP {
  const float* packed_t; const float* saved;
  const float* rgb; const float* density; const float* uncert;
  const float* g_rgb; const float* g_density; const float* g_uncert;
  int64_t n_samples, n_tiles;
  float* dz;
  unsigned int* dz_max;
};

// =====================================================================================================================
// The kernel runs on the hand-scheduled blocks of wide_asm.inc.h (gen_wide_asm.py "DATA GRADIENT"): every gated conversion,
// staging-tile write, read-back and 16-byte record store is issued in an MFMA gap of the layer that consumes the set.
// Per head: NARROW (W3^T d -> set P), WIDE P->Q (records dz of layer 2), WIDE Q->P (records dz
// of layer 1), FINISH (records dz of layer 0).  Sets P / Q live in a[0:255]; nothing seeds them (first MFMA of a tile: C = 0).
// LDS: weight ring 96 KiB | narrow B operand 8 KiB (hi, lo: 16 B per lane each) | four 4 KiB record staging tiles.
// =====================================================================================================================
constexpr int kDgStageOff = kBufs * kChunkFloats;              // floats
constexpr int kDgRecOff = kDgStageOff + 2048;
constexpr int kDgLdsBytes = (kDgRecOff + 4 * 1024) * 4;

struct DgRec { unsigned recw, recr, ro0, ro1; const float* rbase; };
__device__ __forceinline__ DgRec dg_rec_now(const float* block) {
  extern __shared__ __attribute__((aligned(16))) float lds_base[];
  int tid = threadIdx.x;
  asm volatile("" : "+v"(tid));
  const unsigned lane = (unsigned)tid & 63u, j = (unsigned)tid & 31u, hh = ((unsigned)tid >> 5) & 1u;
  const unsigned wave = (unsigned)__builtin_amdgcn_readfirstlane(tid >> 6);
  const unsigned stg = (unsigned)(uintptr_t)AS3(lds_base) + (unsigned)kDgRecOff * 4u + wave * 1024u;
  DgRec c;
  c.recw = stg + ((4u * hh) * 32u + j) * 4u;
  c.recr = stg + lane * 16u;
  c.ro0 = (unsigned)blk_off(0 + (int)(lane >> 3), (int)(lane & 7u) * 4) * 4u;
  c.ro1 = (unsigned)blk_off(8 + (int)(lane >> 3), (int)(lane & 7u) * 4) * 4u;
  const uint64_t b = (uint64_t)(uintptr_t)block;
  c.rbase = reinterpret_cast<const float*>((uint64_t)(unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)b) |
                                           ((uint64_t)(unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(b >> 32)) << 32));
  return c;
}
__device__ __forceinline__ AsmCtx dg_ctx_now(const float* packed_t) {
  extern __shared__ __attribute__((aligned(16))) float lds_base[];
  int tid = threadIdx.x;
  asm volatile("" : "+v"(tid));
  const unsigned lane = (unsigned)tid & 63u;
  const unsigned wave = (unsigned)__builtin_amdgcn_readfirstlane(tid >> 6);
  AsmCtx c;
  const unsigned lds0 = (unsigned)(uintptr_t)AS3(lds_base);
  c.lane16 = lds0 + lane * 16u;
  c.laneoff = lane * 16u;
  c.ldswave = lds0 + wave * 8192u;
  const uint64_t sw = (uint64_t)(uintptr_t)(packed_t + wave * 2048);
  c.stream_lo = (unsigned)sw;
  c.stream_hi = (unsigned)(sw >> 32);
  c.bias0 = 0;
  c.stage0 = lds0 + (unsigned)kDgStageOff * 4u + (unsigned)tid * 16u;
  c.nch = kNumChunksT;
  return c;
}
#define TP_DG_INPUTS(m, isc, r)                                                                                        \
  [g0] "v"(m[0]), [g1] "v"(m[1]), [g2] "v"(m[2]), [g3] "v"(m[3]), [isc] "v"(isc), [recw] "v"(r.recw), [recr] "v"(r.recr), \
      [ro0] "v"(r.ro0), [ro1] "v"(r.ro1), [rbase] "s"(r.rbase)

__device__ __forceinline__ void asm_dg_narrow(Pipe& p, Frag& f, const AsmCtx& c) {
  TP_RING_LOCALS;
  const unsigned stage = c.stage0;
  asm volatile(TP_ASM_DG_NARROW_P : TP_RING(f), TP_RING_STATE : TP_RING_INPUTS(c), [stage] "v"(stage)
               : TP_ASM_CLOBBERS, "memory", "scc");
  TP_RING_DONE;
}
template <bool SRC_P>
__device__ __forceinline__ void asm_dg_wide(Pipe& p, Frag& f, const AsmCtx& c, const uint32_t (&m)[4], float isc, float& dzm,
                                            const DgRec& r) {
  TP_RING_LOCALS;
  const float kinv = kInvScale;
  const unsigned mask = 0xFFFFE000u;
  if constexpr (SRC_P)
    asm volatile(TP_ASM_DG_WIDE_PQ : TP_RING(f), TP_RING_STATE, [dzm] "+v"(dzm)
                 : TP_RING_INPUTS(c), [kinv] "s"(kinv), [mask] "s"(mask), TP_DG_INPUTS(m, isc, r)
                 : TP_ASM_CLOBBERS, "s96", "s97", "memory", "scc");
  else
    asm volatile(TP_ASM_DG_WIDE_QP : TP_RING(f), TP_RING_STATE, [dzm] "+v"(dzm)
                 : TP_RING_INPUTS(c), [kinv] "s"(kinv), [mask] "s"(mask), TP_DG_INPUTS(m, isc, r)
                 : TP_ASM_CLOBBERS, "s96", "s97", "memory", "scc");
  TP_RING_DONE;
}
__device__ __forceinline__ void asm_dg_finish(const uint32_t (&m)[4], float isc, float& dzm, const DgRec& r) {
  const float kinv = kInvScale;
  asm volatile(TP_ASM_DG_FINISH_P : [dzm] "+v"(dzm) : [kinv] "s"(kinv), TP_DG_INPUTS(m, isc, r)
               : TP_ASM_CLOBBERS, "s96", "s97", "memory", "scc");
}

__global__ __launch_bounds__(kThreads, 1) void mlp_dgrad_f16x3_asm_kernel(DgP P) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int j = lane & 31, hh = lane >> 5;
  Pipe p;
  p.stream = P.packed_t; p.lds = lds; p.chunk = 0; p.buf = 0; p.wave = wave; p.lane = lane;
  dma_chunk(p, 0, 0);
  dma_chunk(p, 1, 1);
  __syncthreads();
  Frag frag;
  frag_prime(p, frag);
  float dzm = 0.0f;

  for (int64_t tile = blockIdx.x; tile < P.n_tiles; tile += gridDim.x) {
    const int64_t s_raw = tile * 128 + wave * 32 + j;
    const bool live = s_raw < P.n_samples;
    const int64_t s = live ? s_raw : 0;
    const int64_t gidx = tile * 4 + wave;
    const float* sv = P.saved + gidx * (int64_t)kSavedGroupFloats;
    float* dzg = P.dz + gidx * (int64_t)kDzGroupFloats;
    const auto load_mask = [&](int slot, uint32_t (&mask)[4]) {
      const uint32_t* mk = reinterpret_cast<const uint32_t*>(sv + kMaskOff) + (slot - 1) * 256 + lane;
#pragma unroll
      for (int w = 0; w < 4; ++w) mask[w] = mk[w * 64];
    };

#pragma nounroll
    for (int head = 0; head < 2; ++head) {
      // derivative of the output non-linearities (sigmoid: y(1-y); softplus: 1-exp(-y))
      float d[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      if (live) {
        const int sel = head == 0 ? 1 : 0;          // head 0 = transient (last dim 1), head 1 = static rgb
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const float y = P.rgb[s * 6 + c * 2 + sel];
          d[c] = P.g_rgb[s * 6 + c * 2 + sel] * y * (1.0f - y);
        }
        if (head == 0) {
          d[3] = P.g_density[s * 2 + 1] * (1.0f - expf(-P.density[s * 2 + 1]));
          d[4] = P.g_uncert[s] * (1.0f - expf(-P.uncert[s]));
        }
      }
      float* nb = dzg + (head == 0 ? kDzT3Off : kDzR3Off);
#pragma unroll
      for (int r = 0; r < 16; ++r) nb[blk_off(r + 16 * hh, j)] = (hh == 0 && r < 6) ? d[r < 6 ? r : 0] : 0.0f;
      // per-sample power-of-two scale: largest |d| -> [2^5, 2^6)
      float dmax = 0.0f;
#pragma unroll
      for (int c = 0; c < 6; ++c) dmax = fmaxf(dmax, fabsf(d[c]));
      float sc = 1.0f, isc = 1.0f;
      if (dmax > 1.0e-30f && dmax < 1.0e30f) {
        int e;
        (void)frexpf(dmax, &e);
        sc = ldexpf(1.0f, 6 - e);
        isc = ldexpf(1.0f, e - 6);
      }
      const float isc_live = live ? isc : 0.0f;      // samples past the end record zeros
      // B operand of the narrow chunk: slots 8 h + j of k-step 0 = d[0..5] (lane half 0), zeros elsewhere -> this lane's
      // 16 + 16 bytes of the stage (lane-private: no barrier)
      {
        half2v hp[4], lp[4];
#pragma unroll
        for (int e = 0; e < 8; e += 2) {
          const float v0 = (hh == 0 && e < 6) ? d[e < 6 ? e : 0] * sc : 0.0f;
          const float v1 = (hh == 0 && e + 1 < 6) ? d[e + 1 < 6 ? e + 1 : 0] * sc : 0.0f;
          const float h0 = __uint_as_float(__float_as_uint(v0) & 0xFFFFE000u);
          const float h1 = __uint_as_float(__float_as_uint(v1) & 0xFFFFE000u);
          hp[e >> 1] = __builtin_amdgcn_cvt_pkrtz(h0, h1);
          lp[e >> 1] = __builtin_amdgcn_cvt_pkrtz(v0 - h0, v1 - h1);
        }
        _Float16* stg = reinterpret_cast<_Float16*>(lds + kDgStageOff);
        *reinterpret_cast<half8*>(stg + tid * 8) = pack8(hp);
        *reinterpret_cast<half8*>(stg + 2048 + tid * 8) = pack8(lp);
      }
      const int slot0 = head == 0 ? SV_T2 : SV_R2;
      uint32_t m0[4], m1[4], m2[4];
      load_mask(slot0, m0);
      load_mask(slot0 - 1, m1);
      load_mask(slot0 - 2, m2);
      asm volatile("" ::: "memory");
      asm_dg_narrow(p, frag, dg_ctx_now(P.packed_t));
      asm_dg_wide<true>(p, frag, dg_ctx_now(P.packed_t), m0, isc_live, dzm, dg_rec_now(dzg + (head * 3 + 0) * kBlockFloats));
      asm_dg_wide<false>(p, frag, dg_ctx_now(P.packed_t), m1, isc_live, dzm, dg_rec_now(dzg + (head * 3 + 1) * kBlockFloats));
      asm_dg_finish(m2, isc_live, dzm, dg_rec_now(dzg + (head * 3 + 2) * kBlockFloats));
      asm volatile("" ::: "memory");
    }
  }
  for (int off = 32; off >= 1; off >>= 1) dzm = fmaxf(dzm, __shfl_xor(dzm, off, 64));
  if (lane == 0 && P.dz_max != nullptr && dzm == dzm && dzm < 3.0e38f) atomicMax(P.dz_max, __float_as_uint(dzm));
}

}  // namespace

// launched by tp_mlp_bwd (mlp_bwd.hip) when args->wgrad_precision == TP_MLP_F16X3
int tp_launch_mlp_dgrad_f16x3(const tp_mlp_bwd_args* a, float* dz, unsigned int* dz_max, int grid, hipStream_t stream) {
  if (a->repack) {
    WT w;
    for (int i = 0; i < 16; ++i) w.w[i] = nullptr;
    for (int i = 0; i < 4; ++i) { w.w[W_RGB0 + i] = a->weights.rgb_w[i]; w.w[W_TRANS0 + i] = a->weights.trans_w[i]; }
    hipLaunchKernelGGL(packT16_kernel, dim3(512), dim3(256), 0, stream, w, (_Float16*)a->packed_t);
  }
  static unsigned long long attr_devices = 0;
  if (tp::first_use_on_device(attr_devices)) {
    hipError_t e = hipFuncSetAttribute((const void*)mlp_dgrad_f16x3_asm_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, kDgLdsBytes);
    if (e != hipSuccess) { tp::set_error("hipFuncSetAttribute: %s", hipGetErrorString(e)); return (int)e; }
  }
  DgP D;
  D.packed_t = (const float*)a->packed_t; D.saved = a->saved; D.rgb = a->rgb; D.density = a->density; D.uncert = a->uncert;
  D.g_rgb = a->g_rgb; D.g_density = a->g_density; D.g_uncert = a->g_uncert;
  D.n_samples = (int64_t)a->B * a->R * a->N; D.n_tiles = (D.n_samples + 127) / 128; D.dz = dz; D.dz_max = dz_max;
  hipLaunchKernelGGL(mlp_dgrad_f16x3_asm_kernel, dim3(grid), dim3(kThreads), kDgLdsBytes, stream, D);
  return tp::check_launch("tp_mlp_bwd(dgrad f16x3)");
}

extern "C" size_t tp_mlp_ray_bias_bytes(int B, int R) { return ((size_t)B * 512 + (size_t)B * R * 256) * sizeof(float); }

// launched by tp_mlp_fwd (mlp_fwd.hip) when args->precision == TP_MLP_F16X3 or TP_MLP_F16
int tp_launch_mlp_fwd_f16x3(const tp_mlp_fwd_args* a, int grid, hipStream_t stream) {
  Params P;
  P.packed = (const float*)a->packed;
  P.center = a->center; P.ray = a->ray; P.depth = a->depth; P.points = a->points; P.ray_unit = a->ray_unit;
  P.lat_trans = a->lat_trans; P.lat_light = a->lat_light;
  P.B = a->B; P.R = a->R; P.N = a->N;
  P.n_samples = (int64_t)a->B * a->R * a->N;
  P.n_tiles = (P.n_samples + 127) / 128;
  P.rgb = a->rgb; P.density = a->density; P.uncert = a->uncert; P.saved = a->saved; P.workspace = (float*)a->workspace;
  P.status = a->status; P.act_max = a->act_max; P.ray_bias = a->ray_bias;
  P.density_noise = a->density_noise;
  TP_REQUIRE(a->ray_bias == nullptr || a->density_noise == nullptr, "tp_mlp_fwd: density_noise (train mode) does not go with ray_bias (evaluation)");
  const bool f16 = a->precision == TP_MLP_F16;
  TP_REQUIRE(!f16 || (a->saved == nullptr && a->density_noise == nullptr),
             "tp_mlp_fwd: TP_MLP_F16 is inference only (no activation record `saved`, no `density_noise`)");
  static unsigned long long attr_devices = 0;
  if (tp::first_use_on_device(attr_devices)) {
    hipError_t e = hipFuncSetAttribute((const void*)mlp_fwd_f16x3_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, kLdsBytes);
    if (e == hipSuccess)
      e = hipFuncSetAttribute((const void*)mlp_fwd_f16x3_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, kLdsBytes);
    if (e == hipSuccess)
      e = hipFuncSetAttribute((const void*)mlp_fwd_f16x3_kernel<false, true>, hipFuncAttributeMaxDynamicSharedMemorySize, kLdsBytes);
    if (e == hipSuccess)
      e = hipFuncSetAttribute((const void*)mlp_fwd_f16x3_kernel<false, false, true>, hipFuncAttributeMaxDynamicSharedMemorySize, kLdsBytes);
    if (e == hipSuccess)
      e = hipFuncSetAttribute((const void*)mlp_fwd_f16x3_kernel<false, true, true>, hipFuncAttributeMaxDynamicSharedMemorySize, kLdsBytes);
    if (e != hipSuccess) { tp::set_error("hipFuncSetAttribute: %s", hipGetErrorString(e)); return (int)e; }
  }
  if (a->ray_bias != nullptr) {
    // the ray-bias stream (TP_PACK_RAYBIAS): only the configuration it is laid out for -- a stream packed that way cannot run the
    // plain kernels, so a call outside it is an error, not a fallback
    TP_REQUIRE(a->saved == nullptr && a->center != nullptr && a->N % 128 == 0,
               "tp_mlp_fwd: ray_bias needs input form A, no activation record and N % 128 == 0");
    const int64_t n_rays = (int64_t)a->B * a->R;
    float* img = a->ray_bias;
    float* per_ray = a->ray_bias + (size_t)a->B * 512;
    hipLaunchKernelGGL(rb_image_bias_kernel, dim3(a->B), dim3(256), 0, stream, P.packed, a->lat_trans, a->lat_light, img);
    hipLaunchKernelGGL(rb_ray_bias_kernel, dim3((unsigned)((n_rays + kRbRays - 1) / kRbRays)), dim3(256), 0, stream, P.packed, a->ray,
                       a->R, n_rays, (const float*)img, per_ray);
    if (f16) {
      hipLaunchKernelGGL((mlp_fwd_f16x3_kernel<false, true, true>), dim3(grid), dim3(kThreads), kLdsBytes, stream, P);
      return tp::check_launch("tp_mlp_fwd(f16, ray bias)");
    }
    hipLaunchKernelGGL((mlp_fwd_f16x3_kernel<false, true>), dim3(grid), dim3(kThreads), kLdsBytes, stream, P);
    return tp::check_launch("tp_mlp_fwd(f16x3, ray bias)");
  }
  if (f16) {
    hipLaunchKernelGGL((mlp_fwd_f16x3_kernel<false, false, true>), dim3(grid), dim3(kThreads), kLdsBytes, stream, P);
    return tp::check_launch("tp_mlp_fwd(f16)");
  }
  if (P.saved != nullptr)
    hipLaunchKernelGGL(mlp_fwd_f16x3_kernel<true>, dim3(grid), dim3(kThreads), kLdsBytes, stream, P);
  else
    hipLaunchKernelGGL(mlp_fwd_f16x3_kernel<false>, dim3(grid), dim3(kThreads), kLdsBytes, stream, P);
  return tp::check_launch("tp_mlp_fwd(f16x3)");
}
