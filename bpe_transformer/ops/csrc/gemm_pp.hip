// 8-wave ping-pong bf16 MFMA GEMM for gfx950 (all three GEMMs of a linear layer).
// build-flags: -fno-slp-vectorize   (no packed f32 VALU beside the MFMAs: ops/build.py file_flags)
//
//   C[M, N] = beta * C + sum_r A(i, r) B(r, j)        (fp32 accumulation, bf16 or fp32-slab output)
//
// Each operand is row-major and either K-major (reduction index contiguous:
// X [M][R] or W [N][R]) or MN-major (output index contiguous: dY [R][M],
// W [R][N], X [R][N]).  The forward Y = X W^T is (K, K), the input gradient
// dX = dY W is (K, MN), the weight gradient dW = dY^T X is (MN, MN).
//
// Geometry (guide §5 "The 256² 8-phase template", designed here for both
// operand layouts): 256 x 256 output tile, BK = 64, 512 threads = 8 waves in
// two groups of four.  Group g (waves 4g..4g+3) owns output rows
// [128g, 128g+128); wave wl = w & 3 owns columns [64 wl, 64 wl + 64), i.e.
// 8 x 4 accumulators of mfma_f32_16x16x32_bf16 (128 registers).  The MFMA is
// issued as (B fragment, A fragment) so an accumulator register holds four
// CONSECUTIVE output columns of one row (8-byte packed stores).
//
// Ping-pong: waves w and w+4 share a SIMD.  Group 1 runs one barrier behind
// group 0, so in every barrier interval one wave of each SIMD issues 16 MFMAs
// (one 64 x 32 quadrant of its tile over K = 64, 256 cycles) while its partner
// reads the next quadrant's fragments from LDS and issues LDS-DMA for the
// next K-tile: the matrix pipe alternates between the two waves and never
// waits for LDS.  Quadrant order (m0,n0) (m0,n1) (m1,n1) (m1,n0) reuses one
// operand's fragments between neighbours: 12 / 4 / 8 / 4 ds_read_b128 per
// phase.
//
// Staging: two 64 KiB stages (A image 32 KiB + B image 32 KiB), filled by
// global_load_lds_dwordx4 (LDS-DMA).  K-major images are [256][64] (128-byte
// rows, 16-byte chunk c of row r at c ^ ((r >> 1) & 7): conflict-free for the
// 16x16x32 ds_read_b128 lane groups); MN-major images are cut into [64 k]
// sub-images whose column sets are whole 1-KiB DMA pieces -- eight of 32
// columns for B (sub_off), four of 64 columns for A (sub64_off) -- and read
// with ds_read_b64_tr_b16.  The DMA image is lane-linear, so the swizzle is
// applied to the SOURCE address.
//
// Pipelining: K-tile kt+1 is DMA'd during kt, each wave two 1-KiB pieces in
// every one of the four load sections, in the order the phases of kt+1 read
// them; a section's wait leaves the newest pieces in flight and retires a
// piece before the barrier that precedes its first read (ktile_spread; when
// both operands are MN-major, the weight gradient, the second piece of a pair
// is issued inside the MFMA section).  WAR: a region of the other stage is
// refilled at least one barrier after its last read of kt-1.  Raw s_barrier
// only: __syncthreads() would drain the DMA (guide §5 "Pipelining across
// barriers").
//
// Split-K (weight gradients: R = all tokens) writes fp32 partial tiles to a
// slab reduced by splitk_reduce_kernel (gemm.hip) in a fixed order.
// Epilogue (bf16 output): the tile is staged through the then-free LDS as a
// [256][512 B] image and written back as whole 512-byte rows.
#include "fa_common.h"
#include "kernels.h"

#include <algorithm>
#include <cstdlib>

namespace bpe {
namespace gpp {

constexpr int NT = 512, BT = 256, BK = 64;
constexpr int OPB = 32768;          // one operand image per stage
constexpr int STAGE = 2 * OPB;      // 64 KiB
constexpr int LDS_BYTES = 2 * STAGE;  // 128 KiB
#ifdef BPE_GPP_PHASE_STAMPS
constexpr int LDS_LAUNCH = LDS_BYTES + 8 * 64 * 8;  // + the phase stamps of 8 waves
#else
constexpr int LDS_LAUNCH = LDS_BYTES;
#endif

typedef __attribute__((address_space(3))) void lds_void;
typedef __attribute__((address_space(1))) void gbl_void;

__device__ __forceinline__ int fk(int r) { return (r >> 1) & 7; }

// Source offset (elements, relative to the tile origin) of 16-byte chunk e (0..2047) of a K-major image.
__device__ __forceinline__ int src_off_km(int e, int ld) {
    const int row = e >> 3, lc = (e & 7) ^ fk(row);
    return row * ld + lc * 8;
}

// Tile origin of an operand for K-tile starting at k0 (t0 = first output row/column of the tile).
template <bool KM>
__device__ __forceinline__ const __bf16* tile_ptr(const __bf16* P, long ld, int t0, long k0) {
    return KM ? P + (long)t0 * ld + k0 : P + k0 * ld + t0;
}

// MN-major image: eight [64 k][32 col] sub-images of 4 KiB (64-byte rows), so that
// every set of columns the phases read (a 64-column A block, the 32-column halves of the B blocks) is a whole
// number of 1-KiB DMA pieces.  The 32-byte halves of a row are swapped on odd 8-row groups, which keeps the
// ds_read_b64_tr_b16 reads conflict-free (the 8 rows a 32-lane group reads, r0..r0+3 and r0+8..r0+11, land
// on 8 distinct 32-byte bank groups).
__device__ __forceinline__ int sub_off(int r, int c) {
    return (c >> 5) * 4096 + r * 64 + ((((c >> 4) & 1) ^ ((r >> 3) & 1)) << 5) + ((c & 15) << 1);
}

// Source offset (elements, from the tile origin) of 16-byte chunk e (0..2047) of a sub-image MN-major image:
// sub-image e >> 8, piece (16 k-rows) ((e >> 6) & 3), lane e & 63 -> k-row 16 piece + lane / 4, physical
// 16-byte chunk lane & 3 of the 64-byte row, which holds logical chunk (lane & 3) ^ (2 * bit 3 of the row).
__device__ __forceinline__ int src_off_sub(int e, int ld) {
    const int s = e >> 8, q = (e >> 6) & 3, ln = e & 63;
    const int row = 16 * q + (ln >> 2);
    const int ql = (ln & 3) ^ (((row >> 3) & 1) << 1);
    return row * ld + 32 * s + 8 * ql;
}

// The MN-major A operand (the weight gradient's dY) sits in four
// [64 k][64 col] sub-images of 8 KiB with 128-byte rows instead of eight [64 k][32 col] ones: a 1-KiB DMA piece is
// then 8 whole 128-byte lines of 8 token rows instead of 16 half lines of 16 rows (the A pieces the schedule issues
// are whole 64-column blocks either way, so the schedule is unchanged; B keeps the 32-column halves it needs).  The
// 32-byte segment of a row is swizzled by a64_f(row), which keeps the ds_read_b64_tr_b16 fragment reads
// conflict-free (each 32-lane group reads rows {r0..r0+3, r0+8..r0+11} x one 32-byte segment: 8 distinct bank
// groups; checked exhaustively on the host when the layout was written).
__device__ __forceinline__ int a64_f(int r) { return ((r >> 1) & 1) | (((r >> 3) & 1) << 1); }
__device__ __forceinline__ int sub64_off(int r, int c) {  // byte offset of (k-row r, column c) in that image
    const int cc = c & 63;
    return (c >> 6) * 8192 + r * 128 + (((cc >> 4) ^ a64_f(r)) << 5) + ((cc & 15) << 1);
}
// source offset (elements from the tile origin) of 16-byte image chunk e (0..2047) of that image: sub-image
// e >> 9, piece (8 k-rows) (e >> 6) & 7, lane e & 63 -> k-row 8 piece + lane / 8, physical chunk lane & 7
__device__ __forceinline__ int src_off_sub64(int e, int ld) {
    const int s = e >> 9, q = (e >> 6) & 7, ln = e & 63;
    const int row = 8 * q + (ln >> 3), ch = ln & 7;
    const int lc = (((ch >> 1) ^ a64_f(row)) << 1) | (ch & 1);
    return row * ld + 64 * s + 8 * lc;
}
__device__ __forceinline__ bf16x8 frag_a64(char* img, int tb, int ks, int l) {
    const int r = 32 * ks + 8 * (l >> 4) + ((l & 15) >> 2);
    const int c = tb * 16 + 4 * (l & 3);
    return fa::lds_tr_pair(img, sub64_off(r, c), sub64_off(r + 4, c));
}

// MFMA operand fragment of 16-row/col block tb, k-step ks: lane l gets X[t = 16 tb + (l & 15)][k = 32 ks + 8 (l >> 4) + j].
// KM: a K-major image; otherwise the 32-column sub-images (the MN-major A operand reads frag_a64 instead).
template <bool KM>
__device__ __forceinline__ bf16x8 frag(char* img, int tb, int ks, int l) {
    if constexpr (KM) {
        const int row = tb * 16 + (l & 15);
        const int ch = (4 * ks + (l >> 4)) ^ fk(l & 15);
        return fa::lds_row16(img, row * 128 + (ch << 4));
    } else {
        const int r = 32 * ks + 8 * (l >> 4) + ((l & 15) >> 2);
        const int c = tb * 16 + 4 * (l & 3);
        return fa::lds_tr_pair(img, sub_off(r, c), sub_off(r + 4, c));
    }
}

__device__ __forceinline__ f32x4 mfma16(bf16x8 a, bf16x8 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}

// fp8 operands (F8 != 0, K-major images only).  An fp8 K-tile of 128 values is byte-for-byte the 128-byte row
// segment of a bf16 K-tile of 64, so the staging (DMA, swizzle, fragment reads) is the bf16 kernel's, run on
// the matrices reinterpreted as bf16 rows of half the length.  The two bf16 k-step fragments of a lane (16-byte
// chunks g and 4 + g of its row, g = lane >> 4) together are the 32 bytes one
// v_mfma_scale_f32_16x16x128_f8f6f4 takes per lane: the lanes then cover every k of the 128 exactly once, in
// the same order for both operands, so the products sum over k correctly.  Block scales are 1 (E8M0 127);
// the per-tensor inverse scales are applied in the epilogue.  F8: 1 = e4m3 x e4m3, 2 = e5m2 (A) x e4m3 (B).
typedef int i32x8 __attribute__((ext_vector_type(8)));

__device__ __forceinline__ i32x8 cat8(bf16x8 lo, bf16x8 hi) {
    typedef int i32x4 __attribute__((ext_vector_type(4)));
    const i32x4 a = __builtin_bit_cast(i32x4, lo), b = __builtin_bit_cast(i32x4, hi);
    return i32x8{a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
}

// C += B-operand x A-operand (the kernel issues (B, A) so a register holds 4 consecutive output columns);
// cbsz = format of the first operand (B = the weight, e4m3), blgp = the second's (A: e4m3, or e5m2 for F8 2)
template <int F8>
__device__ __forceinline__ f32x4 mfma_f8(const bf16x8 (&b)[2], const bf16x8 (&a)[2], f32x4 c) {
    return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(cat8(b[0], b[1]), cat8(a[0], a[1]), c, 0,
                                                             F8 == 2 ? 1 : 0, 0, 127, 0, 127);
}

struct Frags {
    bf16x8 a[4][2];  // A (output rows): 4 i-blocks of the current m half x 2 k-steps
    bf16x8 b[2][2];  // B (output cols): 2 j-blocks of the current n half x 2 k-steps
};

__device__ __forceinline__ void bar() {
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
}

// Per-wave phase stamps (a diagnostic variant build: ops.build --variant pstamps -D BPE_GPP_PHASE_STAMPS; read by
// benchmarks/gemm_phase_stamps.py): every wave records s_memtime at four events of each phase of K-tiles
// PST_KT0 .. PST_KT0 + PST_NKT - 1 of the one-tile kernel's K-tile loop -- 0 section start (before its
// fragment reads), 1 after its wait (reads / DMA retired), 2 after the barrier (MFMA section start), 3 after the
// MFMA issue (before the closing barrier) -- into LDS above the two stages (no VMEM traffic, so the kernel's
// vmcnt accounting is untouched), copied to g_gpp_phase at the end for workgroups 0 .. 1023.
#ifdef BPE_GPP_PHASE_STAMPS
constexpr int PST_KT0 = 2, PST_NKT = 4, PST_VALS = PST_NKT * 4 * 4;  // per wave
__device__ long long g_gpp_phase[1024 * 8 * PST_VALS];
__device__ __forceinline__ void pst(int kt, int p, int e) {
    extern __shared__ __attribute__((aligned(16))) char pst_smem[];
    if (kt >= PST_KT0 && kt < PST_KT0 + PST_NKT) {
        const long long t = __builtin_amdgcn_s_memtime();
        const int w = threadIdx.x >> 6;
        if ((threadIdx.x & 63) == 0)
            *reinterpret_cast<long long*>(pst_smem + 2 * 2 * 32768 +
                                          ((w * PST_NKT + kt - PST_KT0) * 16 + 4 * p + e) * 8) = t;
    }
}
#define PST(p, e) pst(kt_idx, p, e)
#else
#define PST(p, e)
#endif

template <bool AK>
__device__ __forceinline__ void load_a(Frags& f, char* img, int g, int m, int l) {
#pragma unroll
    for (int ib = 0; ib < 4; ++ib)
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            if constexpr (AK) f.a[ib][ks] = frag<true>(img, 8 * g + 4 * m + ib, ks, l);
            else f.a[ib][ks] = frag_a64(img, 8 * g + 4 * m + ib, ks, l);
        }
}
template <bool BKM>
__device__ __forceinline__ void load_b(Frags& f, char* img, int wl, int n, int l) {
#pragma unroll
    for (int jb = 0; jb < 2; ++jb)
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) f.b[jb][ks] = frag<BKM>(img, 4 * wl + 2 * n + jb, ks, l);
}

// An empty asm "use" of the accumulators a section just issued MFMAs into (no instruction is emitted).
// Without it hipcc sinks every v_mfma_scale_f32_16x16x128_f8f6f4 of a K-tile past the phase barriers into the
// loop latch (the MFMA results are only read after the loop, the barriers are in other basic blocks, and
// sched_barrier only fences the scheduler inside a block): all 32 fp8 MFMAs of a K-tile then issued in one
// barrier interval and the ping-pong was gone (24 + 8 MFMAs in two sections, three sections empty).  Pinned,
// each section issues its own 8.  The bf16 MFMAs are not sunk (tools/isa_mfma_sections.py checks both).
__device__ __forceinline__ void pin_quadrant(f32x4 (&acc)[8][4], int m, int n, int ib0, int ib1) {
#pragma unroll
    for (int ib = ib0; ib < ib1; ++ib)
#pragma unroll
        for (int jb = 0; jb < 2; ++jb) asm volatile("" ::"v"(acc[4 * m + ib][2 * n + jb]));
}

template <int F8>
__device__ __forceinline__ void mma_quadrant(f32x4 (&acc)[8][4], const Frags& f, int m, int n) {
#pragma unroll
    for (int ib = 0; ib < 4; ++ib)
#pragma unroll
        for (int jb = 0; jb < 2; ++jb) {
            if constexpr (F8 != 0) {
                acc[4 * m + ib][2 * n + jb] = mfma_f8<F8>(f.b[jb], f.a[ib], acc[4 * m + ib][2 * n + jb]);
            } else {
#pragma unroll
                for (int ks = 0; ks < 2; ++ks)
                    acc[4 * m + ib][2 * n + jb] = mfma16(f.b[jb][ks], f.a[ib][ks], acc[4 * m + ib][2 * n + jb]);
            }
        }
    if constexpr (F8 != 0) pin_quadrant(acc, m, n, 0, 4);
}

// Half of a quadrant (i-blocks 2h, 2h+1): the MFMA section can then issue one DMA piece between its halves.
template <int F8>
__device__ __forceinline__ void mma_half(f32x4 (&acc)[8][4], const Frags& f, int m, int n, int h) {
#pragma unroll
    for (int ib = 2 * h; ib < 2 * h + 2; ++ib)
#pragma unroll
        for (int jb = 0; jb < 2; ++jb) {
            if constexpr (F8 != 0) {
                acc[4 * m + ib][2 * n + jb] = mfma_f8<F8>(f.b[jb], f.a[ib], acc[4 * m + ib][2 * n + jb]);
            } else {
#pragma unroll
                for (int ks = 0; ks < 2; ++ks)
                    acc[4 * m + ib][2 * n + jb] = mfma16(f.b[jb][ks], f.a[ib][ks], acc[4 * m + ib][2 * n + jb]);
            }
        }
    if constexpr (F8 != 0) pin_quadrant(acc, m, n, 2 * h, 2 * h + 2);
}

// (Measured and dropped, round 5 (docs/performance.md, ping-pong phase stamps): reading the next K-tile's phase-0 A
// fragments inside phase 3's MFMA section, so phase 0 reads only its B half -- the loaders' lateness at phase 0
// halved in the stamps build, but GPT-2 GEMMs moved -1 to +1 % and the Llama SwiGLU / fp8 GEMMs lost 0.7-1.4 %,
// profiles/bench/ab_r5_prea_fused.log; and issuing the barrier that ends an MFMA section before its last i-block --
// 6-10 % slower, profiles/bench/ab_r5_earlybar_prio.log.)

// ---------------------------------------------------------------------------------------------------------
// The DMA schedule.  A K-tile is four (load section, barrier, MFMA section, barrier) phases.  Issuing the next
// K-tile's 8 LDS-DMA instructions per wave as two bursts of 4 (an earlier form, removed) made those load sections
// longer than the partner wave's 256-cycle MFMA section: each issue costs ~100-185 cycles beside the fragment
// reads, and a build that issued the DMA without ever waiting for it was no faster than one that waited
// (profiles/bench/gpp_diag_b128.log) -- issue placement, not latency.  So every load section issues 2
// pieces, in the order the next K-tile's phases read them:
//   phase 0: A rows [128g, +64)   (read by this group in phase 0 of kt+1)
//   phase 1: half g of B rows {64w' + [0, 32)}   (both groups, phase 0 / 3)
//   phase 2: half g of B rows {64w' + [32, 64)}  (both groups, phase 1)
//   phase 3: A rows [128g + 64, +64)  (this group, phase 2)
// and then waits vmcnt(4): the two newest issues stay in flight, the one issued three load sections ago is
// retired before the barrier that precedes its first read (by either group: group 1 reads a piece one barrier
// after group 0, never before the issuing wave's wait).  WAR: a region of the other buffer is refilled at
// least one barrier after its last read of K-tile kt-1 (A rows: phases 0 / 2, B halves: phases 3 / 1).
// Last K-tile (no issue): vmcnt(2) in phase 0 (B rows [32, 64) of this tile), vmcnt(0) afterwards.

struct SpreadOff {
    int a0[2], a1[2], b0[2], b1[2];  // source offsets (elements from the K-tile origin) of this thread's pieces
    int la0, la1, lb0, lb1;          // wave-uniform LDS chunk index of each piece pair (piece j at + 64 j)
};

// Source offset of chunk e of either image kind: K-major [256][64] (A rows / B rows = output index) or an MN-major
// sub-image layout.  The piece sets line up in all: chunks [1024 g + 512 m, +512) are output rows / columns
// [128 g + 64 m, +64) and chunks {512 w' + 256 h + [0, 256)} the 32-wide half h of block w'.
template <bool AK, bool BKM>
__device__ __forceinline__ SpreadOff spread_offsets(int g, int wl, int l, int lda, int ldb) {
    SpreadOff o;
    o.la0 = 1024 * g + 128 * wl;
    o.la1 = o.la0 + 512;
    o.lb0 = 512 * (2 * g + (wl >> 1)) + 128 * (wl & 1);
    o.lb1 = o.lb0 + 256;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        o.a0[j] = AK ? src_off_km(o.la0 + 64 * j + l, lda) : src_off_sub64(o.la0 + 64 * j + l, lda);
        o.a1[j] = AK ? src_off_km(o.la1 + 64 * j + l, lda) : src_off_sub64(o.la1 + 64 * j + l, lda);
        o.b0[j] = BKM ? src_off_km(o.lb0 + 64 * j + l, ldb) : src_off_sub(o.lb0 + 64 * j + l, ldb);
        o.b1[j] = BKM ? src_off_km(o.lb1 + 64 * j + l, ldb) : src_off_sub(o.lb1 + 64 * j + l, ldb);
    }
    return o;
}

// The in-loop LDS-DMA loads keep the default cache policy: nt, per operand, was measured and dropped
// (profiles/bench/ab_dma_policy_r6.log: on A (activations) -2 to -3 % on the MN x MN weight-gradient GEMMs on one
// box, +1 to +6 % on another, and slower K-major forward / QKV + RoPE / ppt LM-head GEMMs, end to end -0.6-0.9 %;
// on B (weights, re-read every round) slower everywhere).
__device__ __forceinline__ void dma_one(const __bf16* tile0, int off, char* img, int lbase) {
    __builtin_amdgcn_global_load_lds((gbl_void*)(tile0 + off), (lds_void*)(img + lbase * 16), 16, 0, 0);
}

__device__ __forceinline__ void dma_pair(const __bf16* tile0, const int (&off)[2], char* img, int lbase) {
#pragma unroll
    for (int j = 0; j < 2; ++j) dma_one(tile0, off[j], img, lbase + 64 * j);
}

// One K-tile.  `cur` is read, `nxt` is the DMA target (the __restrict__ parameters let the wait-count pass see that
// the fragment reads do not alias the in-flight DMA; without it hipcc drains the DMA before the first read).
// SPLIT (both operands MN-major, the weight gradient): the second piece of each pair is issued by the same wave in
// its MFMA section, between the two halves of the quadrant, so a load section carries one piece; the waits become
// vmcnt(3).  Weight gradients +1-3 %, the other layouts 3 % slower that way (profiles/bench/ab_gpp_dma_split.log).
// FIRST: K-tile 0 of a tile, whose image was retired (vmcnt(0)) before the loop.  Its phases 0-1 would only retire
// pieces of that image, so they wait for LDS only; phases 2-3 retire the first pieces of K-tile 1 (read before any
// wait of K-tile 1) as always.  In the persistent kernel this lets the previous tile's epilogue stores, which
// share the vmcnt counter with the DMA, drain during the first two phases instead of before them.
template <bool AK, bool BKM, int F8>
__device__ __forceinline__ void ktile_spread(char* __restrict__ cur, char* __restrict__ nxt, bool dma,
                                             const __bf16* an, const __bf16* bn, const SpreadOff& so, int g, int wl,
                                             int l, f32x4 (&acc)[8][4], bool first = false, int kt_idx = -1) {
    (void)kt_idx;  // phase stamps builds only
    constexpr bool SPLIT = !AK && !BKM;
    Frags f;
    char* Ac = cur;
    char* Bc = cur + OPB;
    // one phase: fragment reads (done by the caller), pieces of (tile, off, img, lbase), wait, barrier, MFMAs
    // relax: phase 2 (m1, n1) retires nothing that a read before phase 3's barrier needs (its own A rows of K-tile
    // kt + 1 are first read in phase 0 of kt + 1; the group's B halves it issued are retired in phase 3 / phase 0),
    // so it waits vmcnt(6) and leaves the piece pair issued two load sections ago in flight one section longer
    auto phase = [&](const __bf16* t0, const int (&off)[2], char* img, int lb, int m, int n, bool last_nodma_wait2,
                     bool relax = false) {
        const int ph = 2 * m + (m ? 1 - n : n);  // (m0,n0) 0, (m0,n1) 1, (m1,n1) 2, (m1,n0) 3
        (void)ph;
        if (dma) {
            if constexpr (SPLIT) dma_one(t0, off[0], img, lb);
            else dma_pair(t0, off, img, lb);
        }
        if (first && m == 0) {
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        } else if (dma) {
            if constexpr (SPLIT) asm volatile("s_waitcnt vmcnt(3) lgkmcnt(0)" ::: "memory");
            else if (relax) asm volatile("s_waitcnt vmcnt(6) lgkmcnt(0)" ::: "memory");
            else asm volatile("s_waitcnt vmcnt(4) lgkmcnt(0)" ::: "memory");
        } else if (last_nodma_wait2) {
            asm volatile("s_waitcnt vmcnt(2) lgkmcnt(0)" ::: "memory");
        } else {
            asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        }
        PST(ph, 1);
        bar();
        PST(ph, 2);
        if constexpr (SPLIT) {
            mma_half<F8>(acc, f, m, n, 0);
            if (dma) {
                __builtin_amdgcn_sched_barrier(0);
                dma_one(t0, off[1], img, lb + 64);
                __builtin_amdgcn_sched_barrier(0);
            }
            mma_half<F8>(acc, f, m, n, 1);
        } else {
            mma_quadrant<F8>(acc, f, m, n);
        }
        PST(ph, 3);
        bar();
    };
    // phase 0: (m0, n0)
    PST(0, 0);
    load_a<AK>(f, Ac, g, 0, l);
    load_b<BKM>(f, Bc, wl, 0, l);
    phase(an, so.a0, nxt, so.la0, 0, 0, true);
    // phase 1: (m0, n1)
    PST(1, 0);
    load_b<BKM>(f, Bc, wl, 1, l);
    phase(bn, so.b0, nxt + OPB, so.lb0, 0, 1, false);
    // phase 2: (m1, n1)
    PST(2, 0);
    load_a<AK>(f, Ac, g, 1, l);
    phase(bn, so.b1, nxt + OPB, so.lb1, 1, 1, false, true);
    // phase 3: (m1, n0)
    PST(3, 0);
    load_b<BKM>(f, Bc, wl, 0, l);
    phase(an, so.a1, nxt, so.la1, 1, 0, false);
}

// Fused epilogues of the one-tile-per-workgroup kernel.  EPI_SWIGLU_BWD: the GEMM result is da = dY W2 (the
// gradient of a = silu(g) * u); instead of storing da the epilogue reads g and u from gu = [g | u] ([M][2F])
// and writes dgu = [dg | du] -- the SwiGLU backward without the da round trip through HBM.  Same math and
// rounding as swiglu_bwd_kernel (da rounded to bf16 first).
// EPI_SWIGLU_FWD: the forward gu = X [W1; W3]^T with a = silu(g) * u in the epilogue.  A workgroup's 256 output
// columns are 128 columns of g and the SAME 128 columns of u (B rows [128 t, +128) and [F + 128 t, +128) of
// [W1; W3]), so the epilogue writes both halves of gu and the gate a from one tile -- the separate swiglu_fwd
// pass over gu (read 2F, write F per token) disappears.  Same rounding as swiglu_fwd_kernel (a from bf16 g, u).
// Per-workgroup s_memtime stamps (a diagnostic variant build: ops.build --variant stamps -D BPE_GPP_STAMPS; read
// by benchmarks/gemm_stamps.py): slot 0 entry, 1 prologue retired, 2 main loop done, 3 epilogue staged, 4 stores
// issued, 6 work id, 7 hardware XCC id.  Thread 0 writes them (wave 0's view of the workgroup).
#ifdef BPE_GPP_STAMPS
__device__ long long g_gpp_stamps[65536 * 8];
#define GPP_STAMP(i)                                                                                       \
    do {                                                                                                   \
        if (threadIdx.x == 0) g_gpp_stamps[(long)(blockIdx.x & 65535) * 8 + (i)] = __builtin_amdgcn_s_memtime(); \
    } while (0)
#define GPP_STAMP_VAL(i, v)                                                                                \
    do {                                                                                                   \
        if (threadIdx.x == 0) g_gpp_stamps[(long)(blockIdx.x & 65535) * 8 + (i)] = (v);                      \
    } while (0)
#define GPP_STAMP_T(t, i)                                                                                  \
    do {                                                                                                   \
        if (threadIdx.x == 0) g_gpp_stamps[(long)((t) & 65535) * 8 + (i)] = __builtin_amdgcn_s_memtime();    \
    } while (0)
#else
#define GPP_STAMP(i)
#define GPP_STAMP_VAL(i, v)
#define GPP_STAMP_T(t, i)
#endif

// EPI_ROPE: the QKV projection with RoPE on its Q / K columns (output columns [0, rot_cols)), applied to the
// bf16-rounded products exactly as rope_qk_kernel (rope.hip) applies it to the stored activation: interleaved
// pairs, position = row % S, fp32 cos / sin tables [S][D / 2].  Saves the separate in-place pass over Q / K.
// EPI_SWIGLU_FWD8: the fp8 forward [W1; W3] GEMM (e4m3 x e4m3) with the SwiGLU gate AND its two-layout e4m3 cast
// in the epilogue: writes gu (bf16, for the backward), a8 = e4m3(a * scale) [M][F] and a8t [F][M] (the W2 GEMM's
// operands) and folds max |a| into the slot's amax -- the swiglu_cast_fp8 pass over gu (0.43 ms per Llama layer at
// 65 536 tokens) disappears.  Same values, rounding and amax as launch_gemm_fp8 + swiglu_cast_fp8_t (bitwise).
// Persistent kernel only (the a8 tile is transposed through 18 KiB of LDS past the two stages).
enum { EPI_NONE = 0, EPI_SWIGLU_BWD = 1, EPI_SWIGLU_FWD = 2, EPI_ROPE = 3, EPI_SWIGLU_FWD8 = 4 };
constexpr bool is_swf(int e) { return e == EPI_SWIGLU_FWD || e == EPI_SWIGLU_FWD8; }
constexpr int A8T_STRIDE = 144;               // bytes per token row of the a8 transpose tile (conflict-free reads)
constexpr int A8T_BYTES = 128 * A8T_STRIDE;   // one pass: 128 token rows x 128 a columns
// Store policy of the fused epilogues' outputs (MI355X_MICROARCH store flavours): 0 = plain (the line stays in
// the XCD's L2), 1 = sc1 (written through and dropped from L2), 2 = nt.  The outputs are 0.6-1.1 GB streams read
// by later kernels only; kept in L2 they evict the main loop's operand tiles.  Per output, measured per call at
// GPT-2 B 128 (profiles/bench/ab_epilogue_store_policy_r6.log):
constexpr int POL_SWB = 1;     // SwiGLU backward dg / du (sc1: 0.67 vs 0.70-0.71 ms per GPT-2 call)
constexpr int POL_SWF_GU = 2;  // SwiGLU forward gu (nt; sc1 on gu and a: 0.85 vs 0.82 ms)
constexpr int POL_SWF_A = 0;   // SwiGLU forward a
constexpr int POL_ROPE = 1;    // QKV + RoPE output (sc1: 0.426-0.428 vs 0.433-0.434 ms)

// 16-byte store of v at byte offset off from the wave-uniform base (a buffer resource for the cache-policy forms:
// built from uniform values, so it lives in SGPRs -- no waterfall)
template <int POL>
__device__ __forceinline__ void st16(__bf16* base, unsigned off, const u16x8& v) {
#if defined(__HIP_DEVICE_COMPILE__)
    if constexpr (POL == 0) {
        *reinterpret_cast<u16x8*>(reinterpret_cast<char*>(base) + off) = v;
    } else {
        typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
        const auto rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)base, 0, 0x7fffffff, 0x00020000);
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), rsrc, off, 0, POL == 1 ? 16 : 2);
    }
#endif
}
struct Epi {
    const __bf16* gu;
    __bf16* dgu;  // EPI_SWIGLU_BWD: dgu out; EPI_SWIGLU_FWD: gu out
    long ld;      // row stride of gu / dgu (elements)
    int F;
    __bf16* act = nullptr;  // EPI_SWIGLU_FWD: a = silu(g) * u, [M][F]
    long ld_act = 0;
    int prio = 0;  // 1: group 1 (the younger waves 4-7) runs at s_setprio 1 (guide T5, static form)
    const float* sa = nullptr;  // F8: device-resident per-tensor inverse scales of A and B (output x sa x sb)
    const float* sb = nullptr;
    const float* cosT = nullptr;  // EPI_ROPE: [S][D / 2] tables, S, head dim, rotated column count
    const float* sinT = nullptr;
    int S = 0, D = 0, rot_cols = 0;
    uint8_t* a8 = nullptr;        // EPI_SWIGLU_FWD8: a8 [M][F], a8t [F][M] (ld M), the slot's scale and amax bits
    uint8_t* a8t = nullptr;
    long ld_a8t = 0;
    const float* a_scale = nullptr;
    unsigned* a_amax = nullptr;
    int gm = 0;  // tile order (tile_rc): 0 = row-major, gm > 0 = column-major within bands of gm row blocks
};

// Output tile t -> (row block ti, column block tj).  gm 0: row-major.  gm > 0: the tile grid cut into bands of gm
// row blocks, column-major inside a band, so the 32 consecutive work ids of one XCD in a round cover 32 / gm
// columns x gm rows instead of 32 / tiles_n rows x every column: when 256 is a multiple of gm x tiles_n, an XCD
// then keeps the same B column blocks in every round and its L2 holds them, instead of re-reading all of B (3.5-6.3
// MiB at GPT-2 K = 768, more than the 4 MiB L2) every round.
__device__ __forceinline__ void tile_rc(int t, int tiles_m, int tiles_n, int gm, int& ti, int& tj) {
    if (gm <= 0) {
        ti = t / tiles_n;
        tj = t % tiles_n;
        return;
    }
    const int band = t / (gm * tiles_n);
    const int r0 = band * gm;
    const int rows = tiles_m - r0 < gm ? tiles_m - r0 : gm;
    const int wb = t - band * gm * tiles_n;
    ti = r0 + wb % rows;
    tj = wb / rows;
}

// The staging half of epilogue_bf16: this lane's accumulators of tile rows [r0, r0 + 256 / NPASS) rounded to bf16
// into the LDS image at stg.  ADDC (the plain GEMM with beta != 0): beta * C joins the fp32 accumulator here, read
// from c0 (the first output element of the pass) as the 8-byte pieces of the accumulator layout, so the sum is
// rounded to bf16 once -- as gemm.hip and splitk_reduce do.  (Adding C to the staged bf16 value in the write-back
// rounded twice: acc 257, C 1 gave 256.)
template <int F8, bool ADDC>
__device__ __forceinline__ void stage_rows(const f32x4 (&acc)[8][4], char* stg, int g, int wl, int l, int r0,
                                           float osc, const __bf16* c0, long ldc, float beta) {
#if defined(__HIP_DEVICE_COMPILE__)
    // ADDC: buffer loads from the wave-uniform c0 -- one VGPR (this lane's byte offset in the pass) addresses all 32
    // pieces, the (ib, jq) part of the offset is uniform; 64-bit addresses per piece spilled beside the accumulators
    typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
    const auto rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)c0, 0, 0x7fffffff, 0x00020000);
    const unsigned lane_off =
        (unsigned)(((long)(128 * g + (l & 15) - r0) * ldc + 64 * wl + 4 * (l >> 4)) * 2);
#endif
#pragma unroll
    for (int ib = 0; ib < 8; ++ib)
#pragma unroll
        for (int jq = 0; jq < 4; ++jq) {
            const int i = 128 * g + 16 * ib + (l & 15) - r0;
            const int j = 64 * wl + 16 * jq + 4 * (l >> 4);
            f32x4 v = F8 != 0 ? acc[ib][jq] * osc : acc[ib][jq];
            if constexpr (ADDC) {
#if defined(__HIP_DEVICE_COMPILE__)
                const u32x2 w = __builtin_amdgcn_raw_buffer_load_b64(
                    rsrc, lane_off, (unsigned)(((long)(16 * ib) * ldc + 16 * jq) * 2), 0);
                const u16x4 o = __builtin_bit_cast(u16x4, w);
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] += beta * bf2f(o[e]);
#endif
            }
            const u16x4 p = u16x4{f2bf(v[0]), f2bf(v[1]), f2bf(v[2]), f2bf(v[3])};
            *reinterpret_cast<u16x4*>(stg + i * 512 + ((((j >> 3) ^ (i & 15))) << 4) + ((j & 7) << 1)) = p;
        }
}

// bf16 epilogue: the tile is staged through LDS at stg as [256 / NPASS][512 B] images (16-byte chunk c of row i at
// c ^ (i & 15)) and written back as whole rows.  NPASS 1: the whole tile at once (128 KiB, the one-tile kernel);
// NPASS 2: group h's rows [128 h, +128) in pass h through one 64 KiB image (the persistent kernel, whose other
// stage already holds the next tile's K-tile 0).  Raw barriers with LDS-only waits: the stores of a pass stay in
// flight.  TAIL: a barrier after the last pass too (the image is the next tile's DMA target).
template <int EPI, int F8, int NPASS>
__device__ __forceinline__ void epilogue_bf16(const f32x4 (&acc)[8][4], char* stg, int g, int wl, int l, int tid,
                                              int i0, int j0, int jb, __bf16* C, long ldc, float beta, const Epi& ep,
                                              bool tail, int sid, char* xtra = nullptr, float* amx = nullptr) {
    constexpr int RP = BT / NPASS;  // tile rows per pass
    float osc = 1.f;  // F8: the product of the operands' inverse scales (device-resident, one load)
    if constexpr (F8 != 0) osc = ep.sa[0] * ep.sb[0];
#pragma unroll
    for (int h = 0; h < NPASS; ++h) {
        const int r0 = h * RP;  // first tile row of this pass
        if (NPASS == 1 || g == h) {
            if constexpr (EPI == EPI_NONE) {
                const __bf16* c0 = C + (long)(i0 + r0) * ldc + j0;
                if (beta != 0.f) stage_rows<F8, true>(acc, stg, g, wl, l, r0, osc, c0, ldc, beta);
                else stage_rows<F8, false>(acc, stg, g, wl, l, r0, osc, c0, ldc, beta);
            } else {
                stage_rows<F8, false>(acc, stg, g, wl, l, r0, osc, nullptr, 0, 0.f);
            }
        }
        if constexpr (EPI == EPI_SWIGLU_BWD) {
            // every g / u load of this thread's row segments is issued before the barrier (the accumulators are in
            // LDS now, their registers free): one memory round trip per pass instead of one per unrolled group of
            // rows, overlapped with the other waves' staging writes
            constexpr int NQ = 16 / NPASS;
            const int c = tid & 31;
            u16x8 gv[NQ], uv[NQ];
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                const long ro = (long)(i0 + r0 + q * 16 + (tid >> 5)) * ep.ld + j0 + c * 8;
                gv[q] = ld_stream(reinterpret_cast<const u16x8*>(ep.gu + ro));  // read once
                uv[q] = ld_stream(reinterpret_cast<const u16x8*>(ep.gu + ro + ep.F));
            }
            // raw barrier after the staging writes only: __syncthreads() would also wait for the loads (vmcnt(0))
            // before the first row's math; this way row q waits for its own pair (in-order vmcnt) and its math and
            // stores overlap the later rows' loads
            __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0) only
            bar();
            if (h == 0) GPP_STAMP_T(sid, 3);
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                const int i = q * 16 + (tid >> 5);
                const u16x8 v = *reinterpret_cast<const u16x8*>(stg + i * 512 + ((c ^ (i & 15)) << 4));
                const long ro = (long)(i0 + r0 + i) * ep.ld + j0 + c * 8;
                u16x8 dg, du;
#pragma unroll
                for (int e = 0; e < 8; e += 2) {  // pairs on the packed fp32 VALU (same math and rounding)
                    const f32x2 gg = {bf2f(gv[q][e]), bf2f(gv[q][e + 1])}, uu = {bf2f(uv[q][e]), bf2f(uv[q][e + 1])};
                    const f32x2 d = {bf2f(v[e]), bf2f(v[e + 1])};
                    const f32x2 sg = fast_sigmoid2(gg);
                    const f32x2 a = d * (gg * sg), b = d * uu * sg * (1.f + gg * (1.f - sg));
                    du[e] = f2bf(a.x);
                    du[e + 1] = f2bf(a.y);
                    dg[e] = f2bf(b.x);
                    dg[e + 1] = f2bf(b.y);
                }
                // offsets from the tile's first output element (wave-uniform base)
                __bf16* tb = ep.dgu + (long)(i0 + r0) * ep.ld + j0;
                const unsigned o = (unsigned)(((long)i * ep.ld + c * 8) * 2);
                st16<POL_SWB>(tb, o, dg);
                st16<POL_SWB>(tb, o + (unsigned)ep.F * 2, du);
            }
        } else if constexpr (EPI == EPI_SWIGLU_FWD) {
            // row i: g = staged columns [0, 128), u = [128, 256); 16 threads x 16 bytes per 256-byte segment
            __builtin_amdgcn_s_waitcnt(0xc07f);
            bar();
            if (h == 0) GPP_STAMP_T(sid, 3);
            const int c = tid & 15;
#pragma unroll 4
            for (int q = 0; q < 8 / NPASS; ++q) {
                const int i = q * 32 + (tid >> 4);
                const u16x8 gv = *reinterpret_cast<const u16x8*>(stg + i * 512 + ((c ^ (i & 15)) << 4));
                const u16x8 uv = *reinterpret_cast<const u16x8*>(stg + i * 512 + (((16 + c) ^ (i & 15)) << 4));
                u16x8 av;
#pragma unroll
                for (int e = 0; e < 8; e += 2) {  // pairs on the packed fp32 VALU
                    const f32x2 gg = {bf2f(gv[e]), bf2f(gv[e + 1])};
                    const f32x2 a = gg * fast_sigmoid2(gg) * f32x2{bf2f(uv[e]), bf2f(uv[e + 1])};
                    av[e] = f2bf(a.x);
                    av[e + 1] = f2bf(a.y);
                }
                // gu is next read by the backward, long after this step's forward: streaming stores
                __bf16* tg = ep.dgu + (long)(i0 + r0) * ep.ld + jb;
                const unsigned og = (unsigned)(((long)i * ep.ld + c * 8) * 2);
                st16<POL_SWF_GU>(tg, og, gv);
                st16<POL_SWF_GU>(tg, og + (unsigned)ep.F * 2, uv);
                st16<POL_SWF_A>(ep.act + (long)(i0 + r0) * ep.ld_act + jb, (unsigned)(((long)i * ep.ld_act + c * 8) * 2),
                                av);
            }
        } else if constexpr (EPI == EPI_SWIGLU_FWD8) {
            // as EPI_SWIGLU_FWD for gu; a = bf16(silu(g) u) (swiglu_cast_fp8_c128_kernel's values) is cast to e4m3
            // with the slot's scale, stored row-major from registers and, through the a8 tile in LDS (xtra), as
            // a8t; max |a| accumulates in *amx (one atomic per workgroup, by the caller)
            static_assert(NPASS == 2, "the a8 transpose tile covers one 128-row pass");
            __builtin_amdgcn_s_waitcnt(0xc07f);
            bar();
            if (h == 0) GPP_STAMP_T(sid, 3);
            const int c = tid & 15;
            const float sc = ep.a_scale[0];
            float am = *amx;
#pragma unroll 2
            for (int q = 0; q < 8 / NPASS; ++q) {
                const int i = q * 32 + (tid >> 4);
                const u16x8 gv = *reinterpret_cast<const u16x8*>(stg + i * 512 + ((c ^ (i & 15)) << 4));
                const u16x8 uv = *reinterpret_cast<const u16x8*>(stg + i * 512 + (((16 + c) ^ (i & 15)) << 4));
                float v[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const float gg = bf2f(gv[e]);
                    v[e] = bf2f(f2bf(gg * fast_sigmoid(gg) * bf2f(uv[e])));
                    am = fmaxf(am, fabsf(v[e]));
                }
                const uint2 q8 = {pack4_fp8<0>(v[0] * sc, v[1] * sc, v[2] * sc, v[3] * sc),
                                  pack4_fp8<0>(v[4] * sc, v[5] * sc, v[6] * sc, v[7] * sc)};
                __bf16* tg = ep.dgu + (long)(i0 + r0) * ep.ld + jb;
                const unsigned og = (unsigned)(((long)i * ep.ld + c * 8) * 2);
                st16<POL_SWF_GU>(tg, og, gv);
                st16<POL_SWF_GU>(tg, og + (unsigned)ep.F * 2, uv);
                *reinterpret_cast<uint2*>(ep.a8 + (long)(i0 + r0 + i) * ep.F + jb + c * 8) = q8;
                *reinterpret_cast<uint2*>(xtra + i * A8T_STRIDE + c * 8) = q8;
            }
            *amx = am;
            __builtin_amdgcn_s_waitcnt(0xc07f);
            bar();
            // a8t rows jb + 4 f4 + j (j < 4), tokens i0 + r0 + 8 tg .. + 7: 8 words of 4 columns -> 4 x 8 bytes
            const int f4 = tid & 31, tg = tid >> 5;
            unsigned wv[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) wv[k] = *reinterpret_cast<const unsigned*>(xtra + (8 * tg + k) * A8T_STRIDE + 4 * f4);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                unsigned lo = 0, hi = 0;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    lo |= ((wv[k] >> (8 * j)) & 0xffu) << (8 * k);
                    hi |= ((wv[k + 4] >> (8 * j)) & 0xffu) << (8 * k);
                }
                *reinterpret_cast<uint2*>(ep.a8t + (long)(jb + 4 * f4 + j) * ep.ld_a8t + i0 + r0 + 8 * tg) = uint2{lo, hi};
            }
        } else if constexpr (EPI == EPI_ROPE) {
            // this thread's 8 columns are one quarter of a pair block of one head: the cos / sin loads of its rows
            // (positions) are issued before the barrier, like the SwiGLU-backward operands
            constexpr int NQ = 16 / NPASS;
            const int c = tid & 31;
            const int col = j0 + c * 8;
            const bool rot = col < ep.rot_cols;
            const int pb = (col % ep.D) >> 1;  // first pair of the 8 columns
            f32x4 cs[NQ], sn[NQ];
            if (rot) {
#pragma unroll
                for (int q = 0; q < NQ; ++q) {
                    const long pos = (long)((i0 + r0 + q * 16 + (tid >> 5)) % ep.S) * (ep.D >> 1) + pb;
                    cs[q] = *reinterpret_cast<const f32x4*>(ep.cosT + pos);
                    sn[q] = *reinterpret_cast<const f32x4*>(ep.sinT + pos);
                }
            }
            __builtin_amdgcn_s_waitcnt(0xc07f);
            bar();
            if (h == 0) GPP_STAMP_T(sid, 3);
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                const int i = q * 16 + (tid >> 5);
                u16x8 v = *reinterpret_cast<const u16x8*>(stg + i * 512 + ((c ^ (i & 15)) << 4));
                if (rot) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const float a = bf2f(v[2 * j]), b = bf2f(v[2 * j + 1]);
                        v[2 * j] = f2bf(a * cs[q][j] - b * sn[q][j]);
                        v[2 * j + 1] = f2bf(a * sn[q][j] + b * cs[q][j]);
                    }
                }
                st16<POL_ROPE>(C + (long)(i0 + r0) * ldc + j0, (unsigned)(((long)i * ldc + c * 8) * 2), v);
            }
        } else {
            __builtin_amdgcn_s_waitcnt(0xc07f);
            bar();
            if (h == 0) GPP_STAMP_T(sid, 3);
#pragma unroll 4
            for (int q = 0; q < 16 / NPASS; ++q) {
                const int i = q * 16 + (tid >> 5), c = tid & 31;
                const u16x8 v = *reinterpret_cast<const u16x8*>(stg + i * 512 + ((c ^ (i & 15)) << 4));
                *reinterpret_cast<u16x8*>(C + (long)(i0 + r0 + i) * ldc + j0 + c * 8) = v;  // beta * C: added above
            }
        }
        if (h + 1 < NPASS || tail) {  // every read of the image retired before it is rewritten
            __builtin_amdgcn_s_waitcnt(0xc07f);
            bar();
        }
    }
}


template <bool AK, bool BKM, bool SLAB, int EPI = EPI_NONE, int F8 = 0>
__global__ void __launch_bounds__(NT, 1)
gemm_pp_kernel(const __bf16* __restrict__ A, long lda, const __bf16* __restrict__ B, long ldb,
               float* __restrict__ slab, __bf16* __restrict__ C, long ldc, float beta, int M, int N, int R,
               int splits, Epi ep = Epi{}) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, l = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = w >> 2, wl = w & 3;
    // XCD-aware bijective remap: consecutive work ids run on one XCD (guide §5, T1)
    const int nwg = gridDim.x, orig = blockIdx.x;
    const int xcd = orig & 7, qq = nwg >> 3, rr = nwg & 7;
    const int wid = (xcd < rr ? xcd * (qq + 1) : rr * (qq + 1) + (xcd - rr) * qq) + (orig >> 3);
    const int tiles_n = N / BT;
    const int ntiles = (M / BT) * tiles_n;
    const int split = wid / ntiles, tile = wid % ntiles;
    int ti, tj;
    tile_rc(tile, M / BT, tiles_n, ep.gm, ti, tj);
    const int i0 = ti * BT, j0 = tj * BT;
    // B tile origin: EPI_SWIGLU_FWD tiles 128 g columns (+ the matching u columns, offset F rows in B)
    const int jb = is_swf(EPI) ? tj * (BT / 2) : j0;
    const int nkt = R / BK;
    const int kb = (int)((long)split * nkt / splits);
    const int nk = (int)((long)(split + 1) * nkt / splits) - kb;
    GPP_STAMP(0);
    GPP_STAMP_VAL(6, wid);
#ifdef BPE_GPP_STAMPS
    {
        unsigned xcc, hw;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
        GPP_STAMP_VAL(7, (long long)(xcc & 15));
        GPP_STAMP_VAL(5, (long long)hw);
    }
#endif

    if (ep.prio && g == 1) __builtin_amdgcn_s_setprio(1);  // g is wave-uniform (readfirstlane): a scalar branch
    f32x4 acc[8][4];
#pragma unroll
    for (int a = 0; a < 8; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};

    SpreadOff so = spread_offsets<AK, BKM>(g, wl, l, (int)lda, (int)ldb);
    if constexpr (is_swf(EPI)) {
        // group g DMAs B rows [128 g, +128) of the tile: group 1's are the u rows, F - 128 rows further on
        static_assert(BKM, "SwiGLU forward: B = [W1; W3] is K-major");
        if (g == 1) {
            const int du = (ep.F - BT / 2) * (int)ldb;
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                so.b0[j] += du;
                so.b1[j] += du;
            }
        }
    }
    {  // prologue: all of K-tile 0 (this wave's 8 pieces of the schedule), retired before the first read
        const long k0 = (long)kb * BK;
        const __bf16* a0 = tile_ptr<AK>(A, lda, i0, k0);
        const __bf16* b0 = tile_ptr<BKM>(B, ldb, jb, k0);
        dma_pair(a0, so.a0, smem, so.la0);
        dma_pair(b0, so.b0, smem + OPB, so.lb0);
        dma_pair(b0, so.b1, smem + OPB, so.lb1);
        dma_pair(a0, so.a1, smem, so.la1);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        bar();
    }
    GPP_STAMP(1);
    if (g == 1) bar();  // the stagger: group 1 runs one barrier interval behind group 0
    for (int kt = 0; kt < nk; ++kt) {
        char* cur = smem + (kt & 1) * STAGE;
        char* nxt = smem + ((kt + 1) & 1) * STAGE;
        const long k1 = (long)(kb + kt + 1) * BK;
        ktile_spread<AK, BKM, F8>(cur, nxt, kt + 1 < nk, tile_ptr<AK>(A, lda, i0, k1), tile_ptr<BKM>(B, ldb, jb, k1),
                                  so, g, wl, l, acc, false, kt);
    }
    GPP_STAMP(2);
    if (g == 0) bar();
    // every fragment read and LDS-DMA done: the LDS is free for the epilogue.  The builtin (not inline asm)
    // tells the compiler's wait-count model that the DMA has retired; after an asm wait it still counts the
    // LDS-DMA loads as pending, a second kind of VMEM event beside the epilogue's own loads, and then waits
    // vmcnt(0) before the first use of any of them (the SwiGLU-backward epilogue's 32 g / u loads drained
    // completely before the first row's math; now row q waits for its own pair)
    __builtin_amdgcn_s_waitcnt(0x70);  // vmcnt(0) expcnt(7) lgkmcnt(0)
    bar();

    // accumulator (ib, jb) register r of lane l: row i = 128 g + 16 ib + (l & 15), col j = 64 wl + 16 jb + 4 (l >> 4) + r
    if constexpr (SLAB) {
        float* sp = slab + (long)split * M * N;
        float osc = 1.f;  // F8: the operands' inverse scales, applied to each partial (the reduce only sums)
        if constexpr (F8 != 0) osc = ep.sa[0] * ep.sb[0];
#pragma unroll
        for (int ib = 0; ib < 8; ++ib)
#pragma unroll
            for (int jb = 0; jb < 4; ++jb) {
                const long i = i0 + 128 * g + 16 * ib + (l & 15);
                const long j = j0 + 64 * wl + 16 * jb + 4 * (l >> 4);
                *reinterpret_cast<f32x4*>(sp + i * N + j) = F8 != 0 ? acc[ib][jb] * osc : acc[ib][jb];
            }
        GPP_STAMP(4);
    } else {
        epilogue_bf16<EPI, F8, 1>(acc, smem, g, wl, l, tid, i0, j0, jb, C, ldc, beta, ep, false, blockIdx.x);
        GPP_STAMP(4);
    }
#ifdef BPE_GPP_PHASE_STAMPS
    if (blockIdx.x < 1024 && l < PST_VALS)  // each wave its own values (LDS above the stages; written by itself)
        g_gpp_phase[((long)blockIdx.x * 8 + w) * PST_VALS + l] =
            *reinterpret_cast<const long long*>(smem + LDS_BYTES + (w * PST_VALS + l) * 8);
#endif
}


// Persistent form of the bf16 (or fp8) one-pass GEMM: one workgroup per CU walks tiles wid, wid + grid, ... (the
// same tile order as the one-tile kernel's XCD-aware grid).  What it removes, measured with the stamps build at
// GPT-2 B 128 (benchmarks/gemm_stamps.py): a one-tile workgroup spends ~10-12 % of its time in the prologue (K-tile
// 0's round trip) and then ~2-3k cycles pass before the CU's next workgroup runs.  Here the next tile's K-tile 0
// is DMA'd during the last K-tile of the current one (the in-loop prefetch simply continues across the seam), so
// its image is resident before the epilogue; the epilogue stages through the other 64 KiB stage in two passes
// (NPASS 2), and its stores stay in flight into the first two phases of the next tile's K-tile 0 (which wait for
// LDS only); phase 2's vmcnt wait retires them.
// (An earlier persistent form stored the accumulators from registers as 8-byte row pieces during the next tile's
// first load section and lost to the one-tile kernel: 0.74-0.89 vs 1.0 PF/s on the K = 768 forward GEMMs.)
template <bool AK, bool BKM, int EPI, int F8 = 0>
__global__ void __launch_bounds__(NT, 1)
gemm_pp_persist_kernel(const __bf16* __restrict__ A, long lda, const __bf16* __restrict__ B, long ldb,
                       __bf16* __restrict__ C, long ldc, float beta, int M, int N, int R, Epi ep = Epi{}) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, l = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = w >> 2, wl = w & 3;
    const int nwg = gridDim.x, orig = blockIdx.x;
    const int xcd = orig & 7, qq = nwg >> 3, rr = nwg & 7;
    const int wid = (xcd < rr ? xcd * (qq + 1) : rr * (qq + 1) + (xcd - rr) * qq) + (orig >> 3);
    const int tiles_n = N / BT;
    const int ntiles = (M / BT) * tiles_n;
    const int nk = R / BK;
    if (ep.prio && g == 1) __builtin_amdgcn_s_setprio(1);
    SpreadOff so = spread_offsets<AK, BKM>(g, wl, l, (int)lda, (int)ldb);
    if constexpr (is_swf(EPI)) {
        static_assert(BKM, "SwiGLU forward: B = [W1; W3] is K-major");
        if (g == 1) {
            const int du = (ep.F - BT / 2) * (int)ldb;
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                so.b0[j] += du;
                so.b1[j] += du;
            }
        }
    }
    // tile t: output origin (i0, j0) and B origin jb (EPI_SWIGLU_FWD: 128 g columns + the matching u columns)
    auto origin = [&](int t, int& i0, int& j0, int& jb) {
        int ti, tj;
        tile_rc(t, M / BT, tiles_n, ep.gm, ti, tj);
        i0 = ti * BT;
        j0 = tj * BT;
        jb = is_swf(EPI) ? tj * (BT / 2) : j0;
    };
    int t = wid, i0, j0, jb;
    origin(t, i0, j0, jb);
    {  // prologue of the first tile: all of its K-tile 0, retired before the first read
        const __bf16* a0 = tile_ptr<AK>(A, lda, i0, 0);
        const __bf16* b0 = tile_ptr<BKM>(B, ldb, jb, 0);
        dma_pair(a0, so.a0, smem, so.la0);
        dma_pair(b0, so.b0, smem + OPB, so.lb0);
        dma_pair(b0, so.b1, smem + OPB, so.lb1);
        dma_pair(a0, so.a1, smem, so.la1);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        bar();
    }
    int st = 0;  // the stage holding the current K-tile
    f32x4 acc[8][4];
    float amx = 0.f;  // EPI_SWIGLU_FWD8: this thread's max |a| over its tiles
#ifdef BPE_GPP_STAMPS
    unsigned xcc_id, hw_id;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc_id));
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw_id));
#endif
    for (;;) {
        GPP_STAMP_T(t, 0);
#ifdef BPE_GPP_STAMPS
        if (threadIdx.x == 0) {
            g_gpp_stamps[(long)(t & 65535) * 8 + 5] = hw_id;
            g_gpp_stamps[(long)(t & 65535) * 8 + 6] = wid;
            g_gpp_stamps[(long)(t & 65535) * 8 + 7] = xcc_id & 15;
        }
#endif
        const int tn = t + nwg;
        const bool more = tn < ntiles;
        int i0n = i0, j0n = j0, jbn = jb;
        if (more) origin(tn, i0n, j0n, jbn);
#pragma unroll
        for (int a = 0; a < 8; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (g == 1) bar();  // the stagger
        GPP_STAMP_T(t, 1);
        for (int kt = 0; kt < nk; ++kt) {
            char* cur = smem + st * STAGE;
            char* nxt = smem + (st ^ 1) * STAGE;
            const bool last = kt + 1 == nk;
            // the next K-tile of this tile, or K-tile 0 of the next tile
            const __bf16* an = last ? tile_ptr<AK>(A, lda, i0n, 0) : tile_ptr<AK>(A, lda, i0, (long)(kt + 1) * BK);
            const __bf16* bn = last ? tile_ptr<BKM>(B, ldb, jbn, 0) : tile_ptr<BKM>(B, ldb, jb, (long)(kt + 1) * BK);
            ktile_spread<AK, BKM, F8>(cur, nxt, !last || more, an, bn, so, g, wl, l, acc, kt == 0);
            st ^= 1;
        }
        GPP_STAMP_T(t, 2);
        if (g == 0) bar();
        // the next tile's K-tile 0 (stage st) retired; the stage just read (st ^ 1) is free for the staging
        __builtin_amdgcn_s_waitcnt(0x70);
        bar();
        // (Measured and dropped, round 6: the SwiGLU-backward epilogue straight from the accumulators -- no LDS
        // staging, lane pairs swapping halves into 16-byte chunks, every g / u load issued before the first store
        // -- 0.77 vs 0.69 ms, profiles/bench/ab_swiglu_bwd_reg_epilogue_r6.log: each access instruction then covers
        // 16 rows x 2 x 32 B instead of 2 rows x 512 B.)
        epilogue_bf16<EPI, F8, 2>(acc, smem + (st ^ 1) * STAGE, g, wl, l, tid, i0, j0, jb, C, ldc, beta, ep, more,
                                  t, smem + LDS_LAUNCH, &amx);
        GPP_STAMP_T(t, 4);
        if (!more) break;
        t = tn;
        i0 = i0n;
        j0 = j0n;
        jb = jbn;
    }
    if constexpr (EPI == EPI_SWIGLU_FWD8) {  // the workgroup's max: one atomic per workgroup
        float m = amx;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
        float* red = reinterpret_cast<float*>(smem + LDS_LAUNCH);
        __syncthreads();  // every wave is done with the a8 tile
        if (l == 0) red[w] = m;
        __syncthreads();
        if (tid == 0) {
#pragma unroll
            for (int i = 1; i < NT / 64; ++i) m = fmaxf(m, red[i]);
            atomicMax(ep.a_amax, __float_as_uint(m));  // amax >= 0: the bit pattern orders as the float
        }
    }
}

}  // namespace gpp
}  // namespace bpe

using namespace bpe::gpp;

// Static s_setprio 1 for the younger wave group: end to end +0.1-0.6 % (profiles/bench/ab_e2e_gpp_prio.log).
static int prio_mode() { return 1; }

// Persistent kernel (gemm_pp_persist_kernel) for the one-pass bf16 / fp8 GEMMs: 1 = on (one workgroup per CU),
// 0 = the one-tile kernel, n >= 2 = on with at most n workgroups (tests: many tiles per workgroup on small shapes).
static int g_persist = 1;
int gpp_persist_config(int mode) {
    const int prev = g_persist;
    if (mode >= 0) g_persist = mode;
    return prev;
}

// Tile order of the one-pass GEMMs (Epi::gm, tile_rc): 0 = row-major; n > 0 = column-major within bands of n row
// blocks; -2 = auto: bands of 2 row blocks up to 10 column tiles, 4 above.  Measured per GEMM at GPT-2 B 128 and
// Llama s2048 (benchmarks/gemm_tile_order.py, profiles/bench/gemm_tile_order_r6.log): the SwiGLU forward -9 / -10 %,
// the plain W13 forward -4 / -7 %, the Llama SwiGLU backward -3 %, QKV + RoPE -1.5 % at 9 column tiles with 2 (4
// is 2 % slower there).  Set at run time for A/B (gpp_order_config, or BPE_GPP_GM in the environment); the split-K
// weight-gradient launches keep row-major, the fp8 ones too in auto mode (order_fp8).
static int g_gm = [] {
    const char* e = getenv("BPE_GPP_GM");
    return e && *e ? atoi(e) : -2;
}();
int gpp_order_config(int gm) {
    const int prev = g_gm;
    if (gm >= 0 || gm < -1) g_gm = gm < -1 ? -2 : gm;
    return prev;
}
static int order_for(int tiles_n) { return g_gm >= 0 ? g_gm : (tiles_n <= 10 ? 2 : 4); }
// the fp8 one-pass GEMMs stay row-major in auto mode: the Llama fp8 s4096 step ran 0.5 % slower with the bf16 rule
static int order_fp8() { return g_gm >= 0 ? g_gm : 0; }

static int num_cus() {
    static int n[16] = {};
    int dev = 0;
    (void)hipGetDevice(&dev);
    int& c = n[dev & 15];
    if (c == 0 && hipDeviceGetAttribute(&c, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) c = 256;
    return c;
}

// Launch kernel K over `grid` workgroups with LDS_LAUNCH + `extra` bytes of dynamic LDS (more than 64 KiB: opted
// into once per instantiation).  persist: K walks the tile list itself, so the grid is capped at one workgroup per
// CU (g_persist >= 2: a test hook, at most that many workgroups).
template <auto K, typename... Args>
static void launch(bool persist, int grid, int extra, hipStream_t s, Args... args) {
    static bool attr = false;
    if (!attr) {
        (void)hipFuncSetAttribute((const void*)K, hipFuncAttributeMaxDynamicSharedMemorySize, LDS_LAUNCH + extra);
        attr = true;
    }
    if (persist) grid = std::min(grid, g_persist >= 2 ? g_persist : num_cus());
    K<<<grid, NT, LDS_LAUNCH + extra, s>>>(args...);
}

// One-pass GEMM (no split-K) of (M / 256) x (N / 256) tiles: the persistent kernel, or under gpp_persist_config(0)
// the one-tile kernel
template <bool AK, bool BKM, int EPI, int F8 = 0>
static void launch_onepass(const void* a, long lda, const void* b, long ldb, void* c, long ldc, float beta, int M,
                           int N, int R, const Epi& ep, hipStream_t s) {
    const int ntiles = (M / BT) * (N / BT);
    if (g_persist)
        launch<&gemm_pp_persist_kernel<AK, BKM, EPI, F8>>(true, ntiles, 0, s, (const __bf16*)a, lda, (const __bf16*)b,
                                                          ldb, (__bf16*)c, ldc, beta, M, N, R, ep);
    else
        launch<&gemm_pp_kernel<AK, BKM, false, EPI, F8>>(false, ntiles, 0, s, (const __bf16*)a, lda, (const __bf16*)b,
                                                         ldb, (float*)nullptr, (__bf16*)c, ldc, beta, M, N, R, 1, ep);
}

static Epi make_epi(int gm) {
    Epi ep{};
    ep.prio = prio_mode();
    ep.gm = gm;
    return ep;
}

// dgu = swiglu_bwd(dY . W2, gu): A = dY [M][R] (K-major), B = W2 [R][F] (MN-major)
void launch_gemm_pp_swiglu_bwd(const void* dY, long ldy, const void* W2, long ldw, const void* gu, void* dgu,
                               long ldg, int M, int F, int R, hipStream_t s) {
    Epi ep = make_epi(order_for(F / BT));
    ep.gu = (const __bf16*)gu;
    ep.dgu = (__bf16*)dgu;
    ep.ld = ldg;
    ep.F = F;
    launch_onepass<true, false, EPI_SWIGLU_BWD>(dY, ldy, W2, ldw, nullptr, 0, 0.f, M, F, R, ep, s);
}

// gu = X . [W1; W3]^T and a = silu(g) * u (EPI_SWIGLU_FWD): X [M][R], W13 [2F][R] (both K-major)
void launch_gemm_pp_swiglu_fwd(const void* X, long ldx, const void* W13, long ldw, void* gu, long ldg, void* act,
                               long lda_, int M, int F, int R, hipStream_t s) {
    Epi ep = make_epi(order_for(F / (BT / 2)));
    ep.dgu = (__bf16*)gu;
    ep.ld = ldg;
    ep.F = F;
    ep.act = (__bf16*)act;
    ep.ld_act = lda_;
    launch_onepass<true, true, EPI_SWIGLU_FWD>(X, ldx, W13, ldw, nullptr, 0, 0.f, M, 2 * F, R, ep, s);
}

static void set_rope(Epi& ep, const float* cosT, const float* sinT, int S, int D, int rot_cols) {
    ep.cosT = cosT;
    ep.sinT = sinT;
    ep.S = S;
    ep.D = D;
    ep.rot_cols = rot_cols;
}

// qkv = X . Wqkv^T with RoPE on columns [0, rot_cols) (EPI_ROPE): X [M][R], Wqkv [N][R] (both K-major)
void launch_gemm_pp_rope(const void* X, long ldx, const void* W, long ldw, void* C, long ldc, int M, int N, int R,
                         const float* cosT, const float* sinT, int S, int D, int rot_cols, hipStream_t s) {
    Epi ep = make_epi(order_for(N / BT));
    set_rope(ep, cosT, sinT, S, D, rot_cols);
    launch_onepass<true, true, EPI_ROPE>(X, ldx, W, ldw, C, ldc, 0.f, M, N, R, ep, s);
}

// The fp8 launchers pass the fp8 rows as bf16 rows of half the length: R = K / 2 "bf16" elements = K / 128
// K-tiles of 128 fp8, row strides (bytes) / 2.

// C[M][N] (bf16) = (A8 . B8^T) * sa * sb with A8 [M][K], B8 [N][K] fp8 row-major (K-major), row strides in
// bytes; fmt_a 0 = e4m3, 1 = e5m2; B is e4m3.  M, N multiples of 256, K of 128, strides of 16 bytes.
void launch_gemm_fp8(const void* A, long lda, const void* B, long ldb, void* C, long ldc, int M, int N, int K,
                     int fmt_a, const float* sa, const float* sb, hipStream_t s) {
    Epi ep = make_epi(order_fp8());
    ep.sa = sa;
    ep.sb = sb;
    if (fmt_a == 1)
        launch_onepass<true, true, EPI_NONE, 2>(A, lda / 2, B, ldb / 2, C, ldc, 0.f, M, N, K / 2, ep, s);
    else
        launch_onepass<true, true, EPI_NONE, 1>(A, lda / 2, B, ldb / 2, C, ldc, 0.f, M, N, K / 2, ep, s);
}

// qkv = (X8 . Wqkv8^T) * sa * sb (e4m3 x e4m3, K-major) with RoPE on output columns [0, rot_cols) in the epilogue:
// the fp8 QKV projection and the in-place rope_qk_ pass in one kernel (the scaled product is rounded to bf16 and
// rotated exactly as launch_gemm_fp8 + rope_qk_kernel do it)
void launch_gemm_fp8_rope(const void* A, long lda, const void* B, long ldb, void* C, long ldc, int M, int N, int K,
                          const float* sa, const float* sb, const float* cosT, const float* sinT, int S, int D,
                          int rot_cols, hipStream_t s) {
    Epi ep = make_epi(order_fp8());
    ep.sa = sa;
    ep.sb = sb;
    set_rope(ep, cosT, sinT, S, D, rot_cols);
    launch_onepass<true, true, EPI_ROPE, 1>(A, lda / 2, B, ldb / 2, C, ldc, 0.f, M, N, K / 2, ep, s);
}

// gu = (X8 . W13_8^T) * sa * sb (e4m3 x e4m3, K-major; W13_8 = [W1; W3] [2F][K]) with a = silu(g) u cast to e4m3
// (scale a_scale) in both layouts a8 [M][F], a8t [F][M] and max |a| folded into *a_amax (EPI_SWIGLU_FWD8).  M a
// multiple of 256, F of 128, K of 128.  Always the persistent kernel (g_persist >= 2 caps its grid, as elsewhere).
void launch_gemm_fp8_swiglu(const void* A8, long lda, const void* B8, long ldb, void* gu, long ldg, void* a8,
                            void* a8t, int M, int F, int K, const float* sa, const float* sb, const float* a_scale,
                            unsigned* a_amax, hipStream_t s) {
    // bands of 8 row blocks: the Llama fp8 W13 GEMM 1.17 vs 1.32 ms row-major (profiles/bench/fp8_gemm_orders_r6.log)
    Epi ep = make_epi(g_gm >= 0 ? g_gm : 8);
    ep.dgu = (__bf16*)gu;
    ep.ld = ldg;
    ep.F = F;
    ep.sa = sa;
    ep.sb = sb;
    ep.a8 = (uint8_t*)a8;
    ep.a8t = (uint8_t*)a8t;
    ep.ld_a8t = M;
    ep.a_scale = a_scale;
    ep.a_amax = a_amax;
    launch<&gemm_pp_persist_kernel<true, true, EPI_SWIGLU_FWD8, 1>>(
        true, (M / BT) * (F / (BT / 2)), A8T_BYTES, s, (const __bf16*)A8, lda / 2, (const __bf16*)B8, ldb / 2,
        (__bf16*)nullptr, 0L, 0.f, M, 2 * F, K / 2, ep);
}

// C = beta * C + (A8 . B8^T) * sa * sb, split over K into `splits` fp32 partials (slab [splits][M][N]) summed in a
// fixed order by splitk_reduce: the fp8 weight-gradient GEMM (few output tiles, K = all tokens).  C bf16 or fp32.
void launch_gemm_fp8_splitk(const void* A, long lda, const void* B, long ldb, void* C, long ldc, int M, int N, int K,
                            int fmt_a, const float* sa, const float* sb, float beta, int splits, float* slab,
                            int c_f32, hipStream_t s) {
    Epi ep = make_epi(0);
    ep.sa = sa;
    ep.sb = sb;
    const int grid = (M / BT) * (N / BT) * splits;
    if (fmt_a == 1)
        launch<&gemm_pp_kernel<true, true, true, EPI_NONE, 2>>(false, grid, 0, s, (const __bf16*)A, lda / 2,
                                                               (const __bf16*)B, ldb / 2, slab, (__bf16*)nullptr, 0L,
                                                               0.f, M, N, K / 2, splits, ep);
    else
        launch<&gemm_pp_kernel<true, true, true, EPI_NONE, 1>>(false, grid, 0, s, (const __bf16*)A, lda / 2,
                                                               (const __bf16*)B, ldb / 2, slab, (__bf16*)nullptr, 0L,
                                                               0.f, M, N, K / 2, splits, ep);
    splitk_reduce(slab, C, ldc, beta, M, N, splits, c_f32, s);
}

bool gemm_pp_shape_ok(int M, int N, int R, int splits) {
    return M % BT == 0 && N % BT == 0 && R % BK == 0 && splits >= 1 && R / BK >= splits;
}

// The plain bf16 GEMM of one layout pair: split-K partials into the slab (the caller reduces them), or one pass
template <bool AK, bool BKM>
static void launch_pp(const __bf16* a, long lda, const __bf16* b, long ldb, float* slab, __bf16* c, long ldc,
                      float beta, int M, int N, int R, int splits, hipStream_t s) {
    if (slab != nullptr)
        launch<&gemm_pp_kernel<AK, BKM, true>>(false, (M / BT) * (N / BT) * splits, 0, s, a, lda, b, ldb, slab, c, ldc,
                                               beta, M, N, R, splits, make_epi(g_gm >= 0 ? g_gm : 0));
    else
        launch_onepass<AK, BKM, EPI_NONE>(a, lda, b, ldb, c, ldc, beta, M, N, R, make_epi(order_for(N / BT)), s);
}

void launch_gemm_pp(int a_kmajor, int b_kmajor, const void* A, long lda, const void* B, long ldb, void* C, long ldc,
                    float beta, int M, int N, int R, int splits, float* slab, int c_f32, hipStream_t s) {
    const __bf16* a = (const __bf16*)A;
    const __bf16* b = (const __bf16*)B;
    __bf16* c = (__bf16*)C;
#define L(AK, BKM) launch_pp<AK, BKM>(a, lda, b, ldb, slab, c, ldc, beta, M, N, R, splits, s)
    if (a_kmajor) { if (b_kmajor) L(true, true); else L(true, false); }
    else { if (b_kmajor) L(false, true); else L(false, false); }
#undef L
    // splits > 1, or an fp32 C: the kernel wrote fp32 partials; the ordered reduce
    if (slab != nullptr) splitk_reduce(slab, C, ldc, beta, M, N, splits, c_f32, s);
}

// copy the last gemm_pp launch's stamps out (BPE_GPP_STAMPS builds; false otherwise)
// phase stamps of the last one-tile launch: n workgroups x 8 waves x PST_VALS (BPE_GPP_PHASE_STAMPS builds)
bool gpp_read_phase_stamps(long long* host, int n) {
#ifdef BPE_GPP_PHASE_STAMPS
    (void)hipDeviceSynchronize();
    return hipMemcpyFromSymbol(host, HIP_SYMBOL(bpe::gpp::g_gpp_phase), (size_t)n * 8 * PST_VALS * sizeof(long long),
                               0, hipMemcpyDeviceToHost) == hipSuccess;
#else
    (void)host;
    (void)n;
    return false;
#endif
}

bool gpp_read_stamps(long long* host, int n) {
#ifdef BPE_GPP_STAMPS
    (void)hipDeviceSynchronize();
    return hipMemcpyFromSymbol(host, HIP_SYMBOL(bpe::gpp::g_gpp_stamps), (size_t)n * 8 * sizeof(long long), 0,
                               hipMemcpyDeviceToHost) == hipSuccess;
#else
    (void)host;
    (void)n;
    return false;
#endif
}
