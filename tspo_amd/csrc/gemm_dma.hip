// bf16 MFMA GEMM for gfx950 (MI355X), LDS-DMA operand path ("a9", production since round 4): the persistent 256x256x64 four-wave
// kernel that runs every big problem (gemm_bf16_is_big) - whole 256x256 tiles in whole rounds + the 64x64 remainder phase of
// round 5, 256 accumulators per lane in AGPRs under literal names, the fused epilogues out of a[0:255].  gemm_bf16.hip decodes
// the kernel variant and calls gemm_bf16_dma at the end of this file.
// The laboratory around this kernel (schedule A/Bs, an instrumented copy with the no-DMA ablation and the s_memtime probe of the
// K-step, the register-staged kernel of rounds 2-3) is retired: its measurements are DESIGN 4.2-4.4 and profiles/r2_* .. r4_*, its
// code is in git history up to 849d8b5.
#include "gemm_epilogue.h"
#include <type_traits>

typedef __attribute__((ext_vector_type(4))) int i32x4;

namespace {
template <int I, int N, class F>
__device__ __forceinline__ void sfor(F&& f) {
  if constexpr (I < N) {
    f(std::integral_constant<int, I>{});
    sfor<I + 1, N>(static_cast<F&&>(f));
  }
}

// ===========================================================================
// Literal-AGPR MFMA statements: the compiler is kept out of the AGPRs entirely (tests/test_abi.py audits the generated code).
// ===========================================================================
#define A4_ALL_AGPRS                                                                                                     \
  "a0", "a1", "a2", "a3", "a4", "a5", "a6", "a7", "a8", "a9", "a10", "a11", "a12", "a13", "a14", "a15", "a16", "a17", "a18",  \
      "a19", "a20", "a21", "a22", "a23", "a24", "a25", "a26", "a27", "a28", "a29", "a30", "a31", "a32", "a33", "a34", "a35",   \
      "a36", "a37", "a38", "a39", "a40", "a41", "a42", "a43", "a44", "a45", "a46", "a47", "a48", "a49", "a50", "a51", "a52",   \
      "a53", "a54", "a55", "a56", "a57", "a58", "a59", "a60", "a61", "a62", "a63", "a64", "a65", "a66", "a67", "a68", "a69",   \
      "a70", "a71", "a72", "a73", "a74", "a75", "a76", "a77", "a78", "a79", "a80", "a81", "a82", "a83", "a84", "a85", "a86",   \
      "a87", "a88", "a89", "a90", "a91", "a92", "a93", "a94", "a95", "a96", "a97", "a98", "a99", "a100", "a101", "a102",       \
      "a103", "a104", "a105", "a106", "a107", "a108", "a109", "a110", "a111", "a112", "a113", "a114", "a115", "a116", "a117",  \
      "a118", "a119", "a120", "a121", "a122", "a123", "a124", "a125", "a126", "a127", "a128", "a129", "a130", "a131", "a132",  \
      "a133", "a134", "a135", "a136", "a137", "a138", "a139", "a140", "a141", "a142", "a143", "a144", "a145", "a146", "a147",  \
      "a148", "a149", "a150", "a151", "a152", "a153", "a154", "a155", "a156", "a157", "a158", "a159", "a160", "a161", "a162",  \
      "a163", "a164", "a165", "a166", "a167", "a168", "a169", "a170", "a171", "a172", "a173", "a174", "a175", "a176", "a177",  \
      "a178", "a179", "a180", "a181", "a182", "a183", "a184", "a185", "a186", "a187", "a188", "a189", "a190", "a191", "a192",  \
      "a193", "a194", "a195", "a196", "a197", "a198", "a199", "a200", "a201", "a202", "a203", "a204", "a205", "a206", "a207",  \
      "a208", "a209", "a210", "a211", "a212", "a213", "a214", "a215", "a216", "a217", "a218", "a219", "a220", "a221", "a222",  \
      "a223", "a224", "a225", "a226", "a227", "a228", "a229", "a230", "a231", "a232", "a233", "a234", "a235", "a236", "a237",  \
      "a238", "a239", "a240", "a241", "a242", "a243", "a244", "a245", "a246", "a247", "a248", "a249", "a250", "a251", "a252",  \
      "a253", "a254", "a255"

#define A4_FENCE() asm volatile("" ::: A4_ALL_AGPRS)
// accumulator tile (nn, mi) = a[(nn*8 + mi)*4 .. +3]; nn = column tile 0..7 (16 columns each), mi = row tile 0..7
#define A4_MFMA(NN, MI, WF, AF)                                                                              \
  asm volatile("v_mfma_f32_16x16x32_bf16 a[%c2:%c3], %0, %1, a[%c2:%c3]" ::"v"(WF), "v"(AF), "i"(((NN)*8 + (MI)) * 4), \
               "i"(((NN)*8 + (MI)) * 4 + 3))
#define A4_MFMA_Z(NN, MI, WF, AF)   /* first K-half of a tile: C = 0, no zeroing pass over the accumulators */     \
  asm volatile("v_mfma_f32_16x16x32_bf16 a[%c2:%c3], %0, %1, 0" ::"v"(WF), "v"(AF), "i"(((NN)*8 + (MI)) * 4), \
               "i"(((NN)*8 + (MI)) * 4 + 3))
// the same behind a short wait: for operands the compiler may have (re)assembled with VALU moves right in front of the statement
#define A4_MFMA_W(NN, MI, WF, AF)                                                                            \
  asm volatile("s_nop 3\n\tv_mfma_f32_16x16x32_bf16 a[%c2:%c3], %0, %1, a[%c2:%c3]" ::"v"(WF), "v"(AF), "i"(((NN)*8 + (MI)) * 4), \
               "i"(((NN)*8 + (MI)) * 4 + 3))
template <int IDX>
__device__ __forceinline__ float a4_acc_read() {
  float x;
  asm volatile("v_accvgpr_read_b32 %0, a%c1" : "=v"(x) : "i"(IDX));
  return x;
}

// ===========================================================================
// Epilogue out of a[0:255]
// ===========================================================================
// What a 64-column slice of the wave's tile needs from memory besides the residual: bias / folded bias and LayerNorm
// column sums.  Slice 0's copy is requested one K-step BEFORE the epilogue (behind the MFMAs of the tile's last K-step),
// slice 1's at the start of the epilogue - no load latency is exposed for them.  EpiRows: what the lane's 8 ROW blocks need, the
// same for both slices - the (rstd, -mean*rstd) pairs of the LayerNorm-folded forms - requested with slice 0's columns, i.e.
// also one K-step ahead (round 5: they used to be the first thing the epilogue waited for - an L2 round trip per tile exposed).
struct EpiPre { EpiCols ec; };
struct EpiRows { float2 rst[8]; };
template <int EPI>
__device__ __forceinline__ void epi_prefetch(const GemmArgs& g, int n0, int ws, int q4, EpiPre& p) {
  g3_epi_cols<EPI>(g, n0, ws, q4, p.ec);
  if (epi_has_bias(EPI)) {
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) {
      const int n = n0 + ws * 64 + ni * 16 + q4 * 4;
      p.ec.bias[ni] = *reinterpret_cast<const f32x4*>(g.bias + (n < g.N ? n : 0));
    }
  }
}
template <int EPI>
__device__ __forceinline__ void epi_prefetch_rows(const GemmArgs& g, int m0, int wm, int l15, EpiRows& pr) {
#pragma unroll
  for (int mi = 0; mi < 8; ++mi)
    pr.rst[mi] = epi_is_ln(EPI) ? g3_epi_rowstat(g, m0 + wm * 128 + mi * 16 + l15) : make_float2(1.f, 0.f);
}

// The residual tile of the wave comes in 16-byte loads in the STORE mapping (4 lanes cover 64 contiguous bytes of a row) through
// a ring of 8 x 2 registers.  Slice 0's eight row blocks are requested from INSIDE the tile's last K-step (round 5; epi_rload is
// called from the gaps behind its last barrier, one 16-byte load per gap that holds no DMA): the K-half-0 fragment registers are dead there, so the 64 ring registers cost
// nothing, and the first-touch latency of the residual rows (HBM: the residual stream of a whole video fits no cache) runs behind
// the last 40 MFMAs instead of in front of the epilogue.  Buffer loads: one descriptor per tile (origin = the tile's first
// element, range = to the end of the matrix, so rows past M read 0 without a predicate), one per-lane byte offset for the whole
// kernel, the (row block, column pair, slice) part in the scalar offset - no vector arithmetic and no branch inside the K-step.
// (Columns past N - only when N is not a multiple of 256 - read the next row's values; those elements are never stored and
// belong to no stored statistics slice.)
typedef __attribute__((ext_vector_type(4))) unsigned int epi_u32x4;
struct EpiRes { uint4 r[8][2]; __amdgpu_buffer_rsrc_t rs; unsigned lane; };
__device__ __forceinline__ void epi_res_setup(const GemmArgs& g, int m0, int n0, int wm, int wn, int l15, int q4, EpiRes& rr) {
  const long left = ((long)(g.M - m0) * g.N - n0) * 2;
  rr.rs = __builtin_amdgcn_make_buffer_rsrc((void*)(g.R + (size_t)m0 * g.N + n0), 0, (int)(left < 0x40000000L ? left : 0x40000000L),
                                            0x00020000);
  rr.lane = ((unsigned)(wm * 128 + l15) * (unsigned)g.N + (unsigned)(wn * 128 + (q4 & 1) * 16 + (q4 >> 1) * 8)) * 2u;
}
__device__ __forceinline__ void epi_rload(const GemmArgs& g, int slice, int mi, int pr, EpiRes& rr) {   // slice: 0 / 1 of the wave
  const epi_u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rr.rs, rr.lane, (mi * 16 * g.N + slice * 64 + pr * 32) * 2, 0);
  rr.r[mi][pr] = make_uint4(v[0], v[1], v[2], v[3]);
}
__device__ __forceinline__ void epi_rload_rb(const GemmArgs& g, int slice, int mi, EpiRes& rr) {
  epi_rload(g, slice, mi, 0, rr);
  epi_rload(g, slice, mi, 1, rr);
}

// Epilogue of the wave's 128x128 tile held in a[0:255].  Residual forms: rres holds slice 0's residual rows on entry (see above).
// They are added to the accumulators ON THE MATRIX PIPE, in the load's own layout - D = sel x R + C with the 0/1 selection
// fragments of epi_resid_sel, two MFMAs per 16-byte load - one row block AHEAD of the v_accvgpr_reads of the epilogue proper, so
// the vector pipe neither unpacks nor adds nor un-swaps residual values (round 5: 448 of its instructions per tile; the loads of
// round 4's "residual on the matrix pipe" sat in the K-loop and cost more there than they saved here - these do not).  As soon as
// a row block's pair has gone into its MFMAs the registers are re-requested for slice 1.
template <int EPI, bool FULL>
__device__ __forceinline__ void agpr_epilogue(const GemmArgs& g, int m0, int n0, int wm, int wn, int l15, int q4,
                                              const EpiPre& p0, const EpiRows& prow, EpiRes& rres) {
  asm volatile("s_nop 15\n\ts_nop 7" ::: "memory");   // last MFMA's result -> first v_accvgpr_read
  constexpr bool RES = EPI == GE_RESID || EPI == GE_RESID_ST;
  EpiPre p1;
  epi_prefetch<EPI>(g, n0, wn * 2 + 1, q4, p1);
  i32x4 sel0 = {0, 0, 0, 0}, sel1 = {0, 0, 0, 0};
  if (RES) { sel0 = epi_resid_sel(0, l15, q4); sel1 = epi_resid_sel(1, l15, q4); }
  auto radd = [&](auto nhs_, auto mi_) {   // accumulator tiles (nhs * 4 + 0..3, mi) += the residual rows of row block mi, slice nhs
    constexpr int nhs = decltype(nhs_)::value, mi = decltype(mi_)::value;
    sfor<0, 2>([&](auto pr_) {
      constexpr int pr = decltype(pr_)::value;
      const i32x4 rf = {(int)rres.r[mi][pr].x, (int)rres.r[mi][pr].y, (int)rres.r[mi][pr].z, (int)rres.r[mi][pr].w};
      const i32x4 s0 = sel0, s1 = sel1;   // (named copies: clang does not capture a variable that only an asm operand uses)
      A4_MFMA_W(nhs * 4 + 2 * pr, mi, s0, rf);
      A4_MFMA_W(nhs * 4 + 2 * pr + 1, mi, s1, rf);
    });
    A4_FENCE();
    if (nhs == 0) epi_rload_rb(g, 1, mi, rres);
  };
  if (RES) radd(std::integral_constant<int, 0>{}, std::integral_constant<int, 0>{});
  sfor<0, 2>([&](auto nh_) {                          // the wave's two 64-column slices
    constexpr int nhs = decltype(nh_)::value;
    const int ws = wn * 2 + nhs;
    const EpiPre& p = nhs == 0 ? p0 : p1;
    sfor<0, 8>([&](auto mi_) {
      constexpr int mi = decltype(mi_)::value;
      if (RES) {   // the NEXT row block's residual goes onto its accumulators; this block's MFMAs are one row block old
        if constexpr (mi < 7) radd(std::integral_constant<int, nhs>{}, std::integral_constant<int, mi + 1>{});
        else if constexpr (nhs == 0) radd(std::integral_constant<int, 1>{}, std::integral_constant<int, 0>{});
      }
      f32x4 vv[4];
      sfor<0, 4>([&](auto ni_) {
        constexpr int ni = decltype(ni_)::value;
        constexpr int base = ((nhs * 4 + ni) * 8 + mi) * 4;
        vv[ni][0] = a4_acc_read<base>(); vv[ni][1] = a4_acc_read<base + 1>();
        vv[ni][2] = a4_acc_read<base + 2>(); vv[ni][3] = a4_acc_read<base + 3>();
      });
      A4_FENCE();
      g3_epi_row<EPI, true, FULL>(g, vv, p.ec, prow.rst[mi], m0 + wm * 128 + mi * 16 + l15, n0, ws, q4, nullptr);
    });
  });
}

// ===========================================================================
// "a9": the tile, wave layout, AGPR accumulators and epilogue of the round-2 register-staged kernel ("a7"), but the operands reach
// LDS by LDS-DMA (buffer_load_dwordx4 ... lds) in the schedule of the vendor library's hand-written 256x256x64 kernel for this chip
// (hipBLASLt `Custom_Cijk_Alik_Bljk_BBS_..._MT256x256x64_MI16x16x1`, read from its disassembly as a specification;
// DESIGN 4.4): the WHOLE K-step's fragments live in registers (4 x 32 VGPRs), so a ring buffer can be refilled two stages
// ahead as soon as its second K-half has been read into registers - no staging VGPRs, no ds_write, 16 instead of 32 staging
// instructions per wave and K-step:
//   K-step it (buffer cb = it & 1 holds stage it, nb stage it+1 in flight, fa0/fw0 = K-half 0 of stage it):
//     K-half 0 MFMAs | all 16 fragments of K-half 1 (A, W) <- cb | B1: cb may be refilled | DMA A(it+2), W(it+2) -> cb, one every
//                    6 gaps, on through K-half 1
//     K-half 1 MFMAs | ... DMA | vmcnt(n): stage it+1 landed, B3 | fragments of K-half 0 of stage it+1 <- nb
//   (the vendor kernel frees the A and the W region of cb with separate barriers - three per K-step; measured here: two are
//    0.5-2 % faster, ONE - everything behind the middle of the K-step - 5-8 % slower because it bunches the memory instructions)
// The XOR swizzle of the LDS image (chunk c of row r at c ^ (r & 7)) is applied on the global SOURCE address (an LDS-DMA
// destination is lane-linear).  DMA instructions are inline asm: hipcc's wait-count pass does not see them, so its own
// vmcnt waits (epilogue loads / stores) can only over-wait, and the waits that order DMA against the fragment reads are
// written here explicitly.
//
// WHAT goes into WHICH of the 128 gaps between a K-step's MFMAs is a compile-time table (A9Sched): a wave alone on its SIMD
// hides about three issue slots per 16-cycle MFMA, and the measured cost of a K-step follows the densest stretch of its
// memory instructions, not their number (a one-barrier schedule with 32 memory instructions behind 32 consecutive MFMAs ran
// 5-8 % slower than the three-barrier one; s_memtime probe: a barrier costs 20-40 cycles, the vmcnt wait 0).
// Measured (profiles/r5_a_gemm_tail_ab.txt, same box, interleaved): a partial last round of whole tiles costs 0.18-0.48 tile-times
// (not 1: its lone workgroups run on an otherwise idle chip), ONE sub-tile per workgroup 0.10-0.12 (out-proj 16.48 -> 16.12, fc2
// 16.36 -> 16.10 tile-times), THREE (QKV) 0.49 against 0.18, FOUR (fc1) 0.60 against 0.46 - so the remainder phase runs only
// when the left-over tiles make at most one sub-tile per workgroup.
#define A9_TAIL_MAX_SUBTILES 1

enum : int {
  OP_NONE = 0,
  OP_RA1 = 1,    // +j: A fragment j of K-half 1 <- current buffer
  OP_RW1 = 9,    // +j: W fragment j of K-half 1 <- current buffer
  OP_RA0 = 17,   // +j: A fragment j of K-half 0 of the NEXT stage <- other buffer
  OP_RW0 = 25,
  OP_MDA = 33,   // +j: m0 <- LDS address of A piece j, and its DMA
  OP_MDW = 41,
  OP_B1 = 49, OP_B3 = 50
};
struct A9Sched {
  signed char op[128];   // gap after MFMA i of the K-step (0-63: K-half 0, 64-127: K-half 1)
  int vm;                // DMAs of this K-step issued before B3 (-> s_waitcnt vmcnt(vm) waits for the previous K-step's only)
};

// The schedule (round 4; the alternatives measured against it: DESIGN 4.4, profiles/r4_a_gemm_dma_schedules_and_probes.txt): the
// 16 K-half-1 fragments in the first 16 gaps, ONE barrier at gap 24 frees both regions of the buffer, one DMA every 6 gaps from
// gap 25 (A pieces, then W pieces; around B3 and the next stage's reads), B3 at gap 85, the next stage's K-half-0 fragments in
// every second gap behind it.
constexpr A9Sched a9_schedule() {
  A9Sched t{};
  for (int j = 0; j < 8; ++j) { t.op[j] = (signed char)(OP_RA1 + j); t.op[8 + j] = (signed char)(OP_RW1 + j); }
  t.op[24] = OP_B1;
  const int d[16] = {25, 31, 37, 43, 49, 55, 61, 67, 73, 79, 91, 97, 103, 109, 115, 121};
  for (int j = 0; j < 8; ++j) { t.op[d[j]] = (signed char)(OP_MDA + j); t.op[d[8 + j]] = (signed char)(OP_MDW + j); }
  t.op[85] = OP_B3;
  for (int j = 0; j < 8; ++j) { t.op[86 + 2 * j] = (signed char)(OP_RA0 + j); t.op[102 + 2 * j] = (signed char)(OP_RW0 + j); }
  for (int i = 0; i < 128 && t.op[i] != OP_B3; ++i)
    if (t.op[i] >= OP_MDA && t.op[i] < OP_B1) ++t.vm;
  return t;
}
static_assert(a9_schedule().vm == 10, "8 A and 2 W pieces of a K-step are issued before its B3");

// Where the last K-step of a tile issues residual load i (0-15) of the residual forms: behind B3 (gap 85), in gaps without a DMA.
constexpr int a9_resid_slot(int gap) {
  constexpr int at[16] = {86, 87, 89, 93, 95, 99, 101, 105, 107, 111, 113, 117, 119, 123, 125, 127};
  for (int i = 0; i < 16; ++i)
    if (at[i] == gap) return i;
  return -1;
}

// ---------------------------------------------------------------------------------------------------------------------------
// Remainder phase (round 5).  Whole 256x256 tiles are handed out in whole ROUNDS only: XCD set x owns ntile_x tiles, its 32
// workgroups run floor(ntile_x / 32) of them each.  What is left over (out-proj / fc2 of the encoder: 4 112 tiles = 16.06 rounds,
// i.e. 16 tiles for which the persistent loop used to run a 17th round at 1/16 occupancy) is cut into 64x64 SUB-tiles - 16 per
// tile - and spread over ALL workgroups of the launch: no cross-workgroup reduction, every output element keeps its K order
// (bitwise the results of the whole-tile path).  A sub-tile: 4 waves x (16 rows x 64 columns) - the shape g3_epi_row finishes, so
// every epilogue form incl. the per-64-column-slice row statistics works unchanged - operands by LDS-DMA into an 8-deep ring of
// 16 KB stages (the whole 128 KB), 7 stages in flight, one counted vmcnt + one barrier per K-step.
// ---------------------------------------------------------------------------------------------------------------------------
#define A9T_STAGE 16384        // 64 A rows | 64 W rows, 128 B each
#define A9T_DEPTH 8

struct A9Remainder { int total; int pre[9]; int rounds[8]; };   // tiles left over per XCD set (prefix sums), whole rounds per set
__host__ __device__ inline A9Remainder a9_remainder(int tilesM, int tilesN, int ngrp, int nwl) {
  A9Remainder r{};
  const int npset = 8 / ngrp, n_per = tilesN / ngrp;
  for (int x = 0; x < 8; ++x) {
    const int pset = x / ngrp;
    const int panels = tilesM > pset ? (tilesM - pset + npset - 1) / npset : 0;
    const int nt = panels * n_per;
    r.rounds[x] = nt / nwl;
    r.pre[x + 1] = r.pre[x] + nt % nwl;
  }
  r.total = r.pre[8];
  return r;
}

template <int EPI>
__device__ __forceinline__ void a9_tail_subtile(const GemmArgs& g, char* lds, int m_s, int n_s, int wid, int lane) {
  const int l15 = lane & 15, q4 = lane >> 4, rin = lane >> 3, slot = lane & 7;
  const int nk = g.K / GT_BK;
  // waves 0, 1 bring the A rows (pieces 0-7 of a stage), waves 2, 3 the W rows (pieces 8-15): ONE descriptor per wave
  const bool isw = wid >= 2;
  const bf16_t* base = isw ? g.W + (size_t)n_s * g.K : g.A + (size_t)m_s * g.K;
  const long left = (long)(isw ? g.N - n_s : g.M - m_s) * g.K * 2;
  const __amdgpu_buffer_rsrc_t rs =
      __builtin_amdgcn_make_buffer_rsrc((void*)base, 0, (int)(left < 0x40000000L ? left : 0x40000000L), 0x00020000);
  const __amdgpu_buffer_rsrc_t rz = __builtin_amdgcn_make_buffer_rsrc((void*)base, 0, 0, 0x00020000);   // past the last K-step
  const unsigned lane_goff = ((unsigned)rin * (unsigned)g.K + (unsigned)((slot ^ rin) << 3)) * 2u;
  const unsigned piece_stride = 8u * (unsigned)g.K * 2u;
  const unsigned so0 = (unsigned)(wid & 1) * 4u * piece_stride;
  const unsigned lds_w = (unsigned)(size_t)lds + (unsigned)wid * 4096u;
  auto issue = [&](int st) {   // this wave's 4 pieces of stage st -> ring slot st % DEPTH
    const unsigned bb = lds_w + (unsigned)(st & (A9T_DEPTH - 1)) * A9T_STAGE;
    const unsigned vo = lane_goff + (unsigned)st * (GT_BK * 2u);
    const __amdgpu_buffer_rsrc_t r = st < nk ? rs : rz;
#define A9T_PIECE(Q)                                                                                  \
    asm volatile("s_add_u32 m0, %0, %1" ::"s"(bb), "i"((Q) * 1024) : "scc");                             \
    asm volatile("buffer_load_dwordx4 %0, %1, %2 offen lds" ::"v"(vo), "s"(r), "s"(so0 + (Q) * piece_stride) : "memory")
    A9T_PIECE(0); A9T_PIECE(1); A9T_PIECE(2); A9T_PIECE(3);
#undef A9T_PIECE
  };
  // the previous user of the LDS (main loop / previous sub-tile) is done everywhere, and nothing of this wave is in flight
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
#pragma unroll
  for (int st = 0; st < A9T_DEPTH - 1; ++st) issue(st);
  f32x4 acc[4];
#pragma unroll
  for (int ni = 0; ni < 4; ++ni) acc[ni] = (f32x4){0.f, 0.f, 0.f, 0.f};
  const int sw = l15 & 7;
  const int offA = (wid * 16 + l15) * 128, offW = 8192 + l15 * 128;
  for (int kt = 0; kt < nk; ++kt) {
    // stage kt landed (6 younger stages x 4 DMAs may fly) - for every wave; and everybody is done with ring slot (kt - 1) % DEPTH
    asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" ::"i"(4 * (A9T_DEPTH - 2)) : "memory");
    issue(kt + A9T_DEPTH - 1);
    const char* cur = lds + (kt & (A9T_DEPTH - 1)) * A9T_STAGE;
    bf16x8 fa[2], fw[2][4];      // both K-halves first (one LDS latency per K-step), then the 8 MFMAs
#pragma unroll
    for (int kh = 0; kh < 2; ++kh) {
      const int co = ((kh * 4 + q4) ^ sw) << 4;
      fa[kh] = *reinterpret_cast<const bf16x8*>(cur + offA + co);
#pragma unroll
      for (int ni = 0; ni < 4; ++ni) fw[kh][ni] = *reinterpret_cast<const bf16x8*>(cur + offW + ni * 2048 + co);
    }
#pragma unroll
    for (int kh = 0; kh < 2; ++kh)
#pragma unroll
      for (int ni = 0; ni < 4; ++ni)   // inline asm with VGPR accumulators: hipcc must not pick AGPRs in this kernel (it would for the builtin)
        // (s_nop: see epi_resid_mfma - an operand tuple the compiler assembles with v_movs in front of the statement is not interlocked)
        asm volatile("s_nop 3\n\tv_mfma_f32_16x16x32_bf16 %0, %1, %2, %0" : "+v"(acc[ni]) : "v"(fw[kh][ni]), "v"(fa[kh]));
  }
  const int m = m_s + wid * 16 + l15;
  if (EPI == GE_RESID || EPI == GE_RESID_ST) {   // the residual rows onto the accumulators, exactly as the whole-tile epilogue does it
    const i32x4 sel0 = epi_resid_sel(0, l15, q4), sel1 = epi_resid_sel(1, l15, q4);
#pragma unroll
    for (int pr = 0; pr < 2; ++pr) {
      const int n = n_s + (2 * pr + (q4 & 1)) * 16 + (q4 >> 1) * 8;
      const uint4 rv = (m < g.M && n < g.N) ? *reinterpret_cast<const uint4*>(g.R + (size_t)m * g.N + n) : make_uint4(0u, 0u, 0u, 0u);
      const i32x4 rf = {(int)rv.x, (int)rv.y, (int)rv.z, (int)rv.w};
      epi_resid_mfma(acc[2 * pr], sel0, rf);
      epi_resid_mfma(acc[2 * pr + 1], sel1, rf);
    }
  }
  // last MFMA's result -> first VALU read (the hazard recogniser does not see asm MFMAs); the accumulators are operands of the
  // wait so that no read of them can be scheduled in front of it
  asm volatile("s_nop 15\n\ts_nop 7" : "+v"(acc[0]), "+v"(acc[1]), "+v"(acc[2]), "+v"(acc[3])::"memory");
  EpiCols ec;
  g3_epi_cols<EPI>(g, n_s, 0, q4, ec);
  const float2 rst = epi_is_ln(EPI) ? g3_epi_rowstat(g, m) : make_float2(1.f, 0.f);
  g3_epi_row<EPI, false, false>(g, acc, ec, rst, m, n_s, 0, q4, g.bias);
}

// tail: 0 = every tile of an XCD set is a whole tile (the round-4 behaviour: a partial last round); 1 = whole rounds + the
// remainder phase above.  launch_gemm_a9 chooses (g.variant 83 forces 0).
template <int EPI>
__global__ __launch_bounds__(256, 1) void gemm_bf16_a9_kernel(GemmArgs g, int tilesM, int ngrp, int tail) {
  __shared__ __attribute__((aligned(16))) char lds[2 * G3_STAGE];  // the ONLY LDS object
  constexpr A9Sched SC = a9_schedule();
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l15 = lane & 15, q4 = lane >> 4;
  const int wm = wid >> 1, wn = wid & 1;
  const int nk = g.K / GT_BK;   // >= 2
  const int xcd = blockIdx.x & 7, wl = blockIdx.x >> 3, nwl = gridDim.x >> 3;
  const int grp = xcd % ngrp, pset = xcd / ngrp, npset = 8 / ngrp, n_per = g.tilesN / ngrp;
  const int panels = (tilesM - pset + npset - 1) / npset;
  const int ntile_x = panels * n_per;
  const int lim = tail ? (ntile_x / nwl) * nwl : ntile_x;   // tiles of this XCD set that are run as whole tiles
  const int my_tiles = wl < lim ? (lim - wl + nwl - 1) / nwl : 0;
  if (my_tiles == 0 && !tail) return;
  A4_FENCE();   // claims a[0:255] for this kernel
  // (Measured in round 5 and not kept - profiles/r5_e_gemm_epilogue_experiments.txt: workgroup b started b * w / 256 cycles late, w = 8k
  // ... 65k cycles, so that the 256 epilogues of a round of tiles - 33-67 MB of stores and residual loads - do not reach the memory
  // system in the same few microseconds: no shape gets faster at any window, every shape pays the window.  The epilogue is a
  // per-CU limit, not a chip-level burst.)

  if (my_tiles > 0) {
  // ---- LDS-DMA: piece P = wid*8 + q of a region = rows 8P..8P+7 (1 KB); lane (rin, slot) brings global chunk slot ^ rin.
  //      Address split: voffset = lane part + K-step (ONE v_add per K-step), soffset = piece (loop-invariant SGPRs, the same
  //      for A and W), m0 = LDS destination (one s_add with a literal per piece) ----
  const int rin = lane >> 3, slot = lane & 7;
  unsigned lane_goff = ((unsigned)rin * (unsigned)g.K + (unsigned)((slot ^ rin) << 3)) * 2u;
  unsigned piece_stride = 8u * (unsigned)g.K * 2u;
  unsigned lds0 = (unsigned)(size_t)lds + (unsigned)wid * 8192u;
  unsigned soff0 = (unsigned)wid * 8u * piece_stride;
  int d_kt = 0, d_s = wl;   // the stage the NEXT K-step's DMA brings: K-step inside the tile, tile
  auto rsrc_a = [&](int s_) {   // (tiles at or past `lim` - the two stages requested past the last whole tile - get zero-length resources)
    const int m0 = ((s_ / n_per) * npset + pset) * G3_BM;
    const bool in = s_ < lim && m0 < g.M;
    const long r = in ? ((long)(g.M - m0) * g.K * 2) : 0;
    return __builtin_amdgcn_make_buffer_rsrc((void*)(g.A + (size_t)(in ? m0 : 0) * g.K), 0,
                                             (int)(r < 0x40000000L ? r : 0x40000000L), 0x00020000);
  };
  auto rsrc_w = [&](int s_) {
    const int n0 = (grp * n_per + s_ % n_per) * G3_BN;
    const bool in = s_ < lim && n0 < g.N;
    const long r = in ? ((long)(g.N - n0) * g.K * 2) : 0;
    return __builtin_amdgcn_make_buffer_rsrc((void*)(g.W + (size_t)(in ? n0 : 0) * g.K), 0,
                                             (int)(r < 0x40000000L ? r : 0x40000000L), 0x00020000);
  };
  __amdgpu_buffer_rsrc_t a_rs = rsrc_a(d_s), w_rs = rsrc_w(d_s);
  auto adv_d = [&]() {
    if (++d_kt == nk) {
      asm volatile("" ::: "memory");   // keeps the tile switch (two divisions, two descriptors) a BRANCH: if-converted it runs every K-step
      d_kt = 0; d_s += nwl; a_rs = rsrc_a(d_s); w_rs = rsrc_w(d_s);
    }
  };
  // (named copies inside the lambdas: clang does not capture a variable that only an asm operand uses)
  auto set_m0 = [&](auto q_, auto isw_, unsigned bufbase) {
    constexpr int off = decltype(q_)::value * 1024 + (decltype(isw_)::value ? G3_BM * 128 : 0);
    const unsigned b = bufbase;
    asm volatile("s_add_u32 m0, %0, %1" ::"s"(b), "i"(off) : "scc");
  };
  auto dma = [&](auto q_, auto isw_, unsigned voff) {
    constexpr int q = decltype(q_)::value;
    constexpr bool isw = decltype(isw_)::value;
    const unsigned vo = voff, so = soff0 + q * piece_stride;
    const __amdgpu_buffer_rsrc_t rs = isw ? w_rs : a_rs;
    // default cache policy on purpose: `nt` on the A or the W stream cuts the QKV form's L2-side fetch by a third (3.7 -> 2.5 GB per
    // launch) and is 2-6 % SLOWER on every shape; sc1 / sc0 sc1 change nothing (profiles/r4_g_fetch_calibration_and_cache_policy.txt)
    asm volatile("buffer_load_dwordx4 %0, %1, %2 offen lds" ::"v"(vo), "s"(rs), "s"(so) : "memory");
  };

  // ---- fragments: both K-halves of a stage, A and W: 4 x 8 x 4 VGPRs ----
  const int sw = l15 & 7;
  const int fbaseA = (wm * 128 + l15) * 128, fbaseW = G3_BM * 128 + (wn * 128 + l15) * 128;
  const int co0 = (q4 ^ sw) << 4, co1 = ((4 + q4) ^ sw) << 4;
  i32x4 fa0[8], fa1[8], fw0[8], fw1[8];
  auto ldfrag = [&](const char* p) { return *reinterpret_cast<const i32x4*>(p); };

  // ---- prologue: stages 0 and 1 in flight, stage 0 landed, its K-half 0 in registers ----
  sfor<0, 2>([&](auto b_) {
    const unsigned vo = lane_goff + (unsigned)d_kt * (GT_BK * 2u), bb = lds0 + decltype(b_)::value * G3_STAGE;
    sfor<0, 8>([&](auto q_) {
      set_m0(q_, std::false_type{}, bb); dma(q_, std::false_type{}, vo);
      set_m0(q_, std::true_type{}, bb); dma(q_, std::true_type{}, vo);
    });
    adv_d();
  });
  asm volatile("s_waitcnt vmcnt(16)\n\ts_barrier" ::: "memory");
#pragma unroll
  for (int i = 0; i < 8; ++i) { fa0[i] = ldfrag(lds + fbaseA + i * 2048 + co0); fw0[i] = ldfrag(lds + fbaseW + i * 2048 + co0); }

  int it = 0, c_s = wl;
  constexpr bool RES = EPI == GE_RESID || EPI == GE_RESID_ST;
  EpiRes rres;   // (the residual forms: slice 0's rows, requested from the last K-step of the tile)
  auto kstep = [&](auto zero_, auto last_) {
    constexpr bool ZERO = decltype(zero_)::value, LAST = decltype(last_)::value;
    const int cb = it & 1;
    const char* cur = lds + cb * G3_STAGE;
    const char* nxt = lds + (cb ^ 1) * G3_STAGE;
    const unsigned vo = lane_goff + (unsigned)d_kt * (GT_BK * 2u), bb = lds0 + (unsigned)cb * G3_STAGE;
    sfor<0, 16>([&](auto grp8_) {   // 16 groups of 8 MFMAs: group nn = grp8 & 7 of K-half grp8 >> 3 (see below for what a group walks)
      constexpr int kh = decltype(grp8_)::value >> 3, nn = decltype(grp8_)::value & 7;
      sfor<0, 8>([&](auto mi_) {
        constexpr int mi = decltype(mi_)::value;
        constexpr int gap = kh * 64 + nn * 8 + mi;
        constexpr int op = SC.op[gap];
        {
          // Issue order of a K-half's 64 MFMAs (round 5): group g keeps ONE A-row fragment and walks the eight W fragments, up in
          // even groups and down in odd ones, so that every MFMA shares an operand register quad with the one before it - also across
          // the group boundary, where the straight order (W fragment fixed, A fragments 0..7, then both change) switched both.  Same
          // accumulation order per output, bitwise the same results; +0.4 % frames/s in 9 of 9 alternating same-box rounds against
          // the straight order, three zig-zag forms alike (profiles/r5_e_gemm_epilogue_experiments.txt #6) - the chip is limited by
          // power under this kernel, and operand traffic is power.
          constexpr int wi = (nn & 1) ? 7 - mi : mi;
          const i32x4 wf = kh ? fw1[wi] : fw0[wi], af = kh ? fa1[nn] : fa0[nn];
          if (ZERO && kh == 0) A4_MFMA_Z(wi, nn, wf, af); else A4_MFMA(wi, nn, wf, af);
        }
        if constexpr (op >= OP_RA1 && op < OP_RA1 + 8) fa1[op - OP_RA1] = ldfrag(cur + fbaseA + (op - OP_RA1) * 2048 + co1);
        if constexpr (op >= OP_RW1 && op < OP_RW1 + 8) fw1[op - OP_RW1] = ldfrag(cur + fbaseW + (op - OP_RW1) * 2048 + co1);
        if constexpr (!LAST && op >= OP_RA0 && op < OP_RA0 + 8) fa0[op - OP_RA0] = ldfrag(nxt + fbaseA + (op - OP_RA0) * 2048 + co0);
        if constexpr (!LAST && op >= OP_RW0 && op < OP_RW0 + 8) fw0[op - OP_RW0] = ldfrag(nxt + fbaseW + (op - OP_RW0) * 2048 + co0);
        // last K-step of a tile: no next-stage fragments (the epilogue comes first) - the residual forms request the 16 residual
        // loads of slice 0 there instead (row block by row block, the order the epilogue consumes them), into the registers K-half
        // 0's fragments have left: one load per gap that holds no DMA, from the barrier to the end of the K-step
        if constexpr (LAST && RES) {
          constexpr int ri = a9_resid_slot(gap);
          if constexpr (ri >= 0) epi_rload(g, 0, ri >> 1, ri & 1, rres);
        }
        if constexpr (op >= OP_MDA && op < OP_MDA + 8) {
          set_m0(std::integral_constant<int, op - OP_MDA>{}, std::false_type{}, bb);
          dma(std::integral_constant<int, op - OP_MDA>{}, std::false_type{}, vo);
        }
        if constexpr (op >= OP_MDW && op < OP_MDW + 8) {
          set_m0(std::integral_constant<int, op - OP_MDW>{}, std::true_type{}, bb);
          dma(std::integral_constant<int, op - OP_MDW>{}, std::true_type{}, vo);
        }
        if constexpr (op == OP_B1) {   // every wave holds its K-half-1 fragments of this stage -> both regions may be refilled
          asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
          __builtin_amdgcn_s_waitcnt(0xC07F);
        }
        if constexpr (op == OP_B3)   // this wave's pieces of stage it+1 have landed (SC.vm younger DMAs may fly) -> everybody's
          asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" ::"i"(SC.vm) : "memory");
      });
      A4_FENCE();
    });
    adv_d();
    ++it;
  };

  for (int t = 0; t < my_tiles; ++t) {
    const int m0 = ((c_s / n_per) * npset + pset) * G3_BM, n0 = (grp * n_per + c_s % n_per) * G3_BN;
    kstep(std::true_type{}, std::false_type{});
    for (int kt = 1; kt < nk - 1; ++kt) kstep(std::false_type{}, std::false_type{});
    EpiPre p0;                                                 // slice 0's epilogue inputs arrive behind the last K-step
    EpiRows prow;                                              // and so do the row statistics of the LayerNorm-folded forms
    epi_prefetch<EPI>(g, n0, wn * 2, q4, p0);
    epi_prefetch_rows<EPI>(g, m0, wm, l15, prow);
    if (RES) epi_res_setup(g, m0, n0, wm, wn, l15, q4, rres);
    kstep(std::false_type{}, std::true_type{});
    if (m0 + G3_BM <= g.M && n0 + G3_BN <= g.N) agpr_epilogue<EPI, true>(g, m0, n0, wm, wn, l15, q4, p0, prow, rres);
    else agpr_epilogue<EPI, false>(g, m0, n0, wm, wn, l15, q4, p0, prow, rres);
    c_s += nwl;
    const char* nbuf = lds + (it & 1) * G3_STAGE;              // the next tile's first fragments, behind the epilogue
#pragma unroll
    for (int i = 0; i < 8; ++i) { fa0[i] = ldfrag(nbuf + fbaseA + i * 2048 + co0); fw0[i] = ldfrag(nbuf + fbaseW + i * 2048 + co0); }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the two stages requested past the last tile (zero-length resources)
  }

  if (tail) {   // ---- remainder phase: the left-over tiles of all XCD sets as 64x64 sub-tiles over all workgroups ----
    const A9Remainder rm = a9_remainder(tilesM, g.tilesN, ngrp, nwl);
    for (int j = blockIdx.x; j < rm.total * 16; j += gridDim.x) {
      const int tt = j >> 4, sub = j & 15;
      int x = 0;
#pragma unroll
      for (int i = 1; i < 8; ++i) x += tt >= rm.pre[i] ? 1 : 0;
      int rx = 0;
#pragma unroll
      for (int i = 0; i < 8; ++i) rx = i == x ? rm.rounds[i] : rx;
      int px = 0;
#pragma unroll
      for (int i = 0; i < 8; ++i) px = i == x ? rm.pre[i] : px;
      const int s = rx * nwl + (tt - px);
      const int m0 = ((s / n_per) * npset + x / ngrp) * G3_BM, n0 = ((x % ngrp) * n_per + s % n_per) * G3_BN;
      const int m_s = m0 + (sub >> 2) * 64, n_s = n0 + (sub & 3) * 64;
      if (m_s < g.M && n_s < g.N) a9_tail_subtile<EPI>(g, lds, m_s, n_s, wid, lane);   // (uniform per workgroup)
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the zero-length stages requested past the last K-step
  }
}

template <int EPI>
int launch_gemm_a9(GemmArgs g, hipStream_t st) {
  const int tilesM = (g.M + G3_BM - 1) / G3_BM;
  g.tilesN = (g.N + G3_BN - 1) / G3_BN;
  g.nwg = tilesM * g.tilesN;
  const int ngrp = ((double)g.N * g.K * 2.0 > 4.0e6 && g.tilesN >= 8 && g.tilesN % 2 == 0) ? 2 : 1;
  // remainder phase when a partial last round exists, every XCD set has whole rounds to run, and the left-over tiles make at
  // most A9_TAIL_MAX_SUBTILES 64x64 sub-tiles per workgroup (beyond that the partial round of whole tiles is cheaper: see above)
  const A9Remainder rm = a9_remainder(tilesM, g.tilesN, ngrp, 32);
  int min_rounds = rm.rounds[0];
  for (int x = 1; x < 8; ++x) min_rounds = rm.rounds[x] < min_rounds ? rm.rounds[x] : min_rounds;
  const int tail = (g.variant != 83 && rm.total > 0 && min_rounds >= 1 && rm.total * 16 <= A9_TAIL_MAX_SUBTILES * 256) ? 1 : 0;
  hipLaunchKernelGGL((gemm_bf16_a9_kernel<EPI>), dim3(256), dim3(256), 0, st, g, tilesM, ngrp, tail);
  return tspo::check_launch("gemm_bf16_a9");
}
}  // namespace

int tspo::gemm_bf16_dma(int epi, const GemmArgs& g, hipStream_t st) {
  if (g.K < 2 * GT_BK) return tspo::set_err(TSPO_EINVAL, "gemm_dma: K=%d too small for the DMA kernel", g.K);
  switch (epi) {
    case GE_BIAS: return launch_gemm_a9<GE_BIAS>(g, st);
    case GE_GELU: return launch_gemm_a9<GE_GELU>(g, st);
    case GE_RESID: return launch_gemm_a9<GE_RESID>(g, st);
    case GE_F32: return launch_gemm_a9<GE_F32>(g, st);
    case GE_PATCH: return launch_gemm_a9<GE_PATCH>(g, st);
    case GE_BIAS_LN: return launch_gemm_a9<GE_BIAS_LN>(g, st);
    case GE_GELU_LN: return launch_gemm_a9<GE_GELU_LN>(g, st);
    case GE_BIAS_LN_HM: return launch_gemm_a9<GE_BIAS_LN_HM>(g, st);
    case GE_RESID_ST: return launch_gemm_a9<GE_RESID_ST>(g, st);
  }
  return tspo::set_err(TSPO_EINVAL, "gemm_dma: bad epilogue %d", epi);
}
