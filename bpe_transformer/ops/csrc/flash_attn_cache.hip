// Flash prefill over the KV cache, gfx950 (MI355X): attention of T new tokens per sequence whose keys are the
// cache slabs and whose causal diagonal starts at the device-side position.
// build-flags: -fno-slp-vectorize   (no packed f32 VALU beside the MFMAs: ops/build.py file_flags)
//
//   q [B*T, H*D] (RoPE already applied: kv_append's output), caches K / V [B, Hkv, Lmax, D] with the new tokens
//   already written at pos[b] .. pos[b] + T - 1:
//   o[b*T + t, h] = softmax(q . K[b, h / G, :n]^T * scale) . V[b, h / G, :n],  n = min(pos[b] + t, Lmax - 1) + 1
// The row of a token at or past Lmax (dropped by kv_append) is unspecified.
//
// decode_attn (decode_attn.hip) serves up to 8 query rows per kv head on the VALU; a second turn of a conversation,
// a chunk of a long prompt or a slot refill brings hundreds.  This is fa_fwd_kernel's geometry (flash_attn_fwd.hip:
// 4 waves x 32 query rows, swapped S^T = K.Q^T with the query on the lane, online softmax in log2 units with the
// deferred rescale, the fp32 score tile reused as the B operand of O^T += V^T.P^T) over the cache:
//   * the query rows of a workgroup are (token, group head) pairs of ONE kv head, as in decode_attn_kernel: row r
//     is token r / G of head hk * G + r % G, in blocks of 128 rows.  K and V are read once for the G heads, and a
//     small T under GQA still fills the MFMA tiles.  The causal limit of row r is pos[b] + r / G;
//   * a (b, hk) slab is contiguous, so the row stride is D and a 64-key tile is one contiguous block: K / V tiles
//     come by LDS-DMA through buffer resources (fa_common.h dma_tile64_buf) into a double buffer, one barrier per
//     tile.  The buffer extent is L = min(pos[b] + T, Lmax) rows: rows from L on -- stale or never written, NaN
//     for all the kernel knows -- read as zeros (a NaN in a V row times P = 0 inside the MFMA would still be NaN)
//     and their scores are masked to -inf;
//   * key tiles wholly above a wave's last row are skipped; only tiles that reach a wave's first limit (diagonal or
//     tail tiles) take the per-score mask.  Key 0 is visible to every row, so the first tile always holds a finite
//     score and the running max is finite from there on;
//   * pos is read on the device (stride 0: shared, 1: per sequence) and the grid depends on B, Hkv, G * T only:
//     the launch is shape-static.  No atomics, no split of the key range: deterministic.  A very long cache with a
//     tiny T has few workgroups; that case stays on decode_attn (models/generation.py routes it).
//
// The kernel body is written once against the cache format (kv_cache.h: Bf16Cache / Fp8Cache).  Over the e4m3 cache
// (kv_fp8.hip: rows of D bytes, one power-of-two fp32 scale each) the result is, bit for bit, that of the bf16
// instantiation on the cache kv_dequant would write -- DESIGN (a) of the two that give those bits: a per-tile
// conversion pass.  The 64 x D byte tile and its 64 K and 64 V scales come by LDS-DMA into a staging image (fa_common.h
// dma_bytes64_buf / dma_scales64_buf; extents L * D and L * 4 bytes, so bytes AND scales from row L on read as zeros
// -- a stale NaN scale there would otherwise reach the output through 0 * NaN; a NaN scale below L is a non-finite
// row of the sequence and gives NaN as in the bf16 cache).  All four waves then convert it with kv_dequant's own
// arithmetic, f2bf(e4m3 * s), into the swizzled bf16 image the DMA of the bf16 instantiation would have left, and
// everything after that is the same code on the same bits.  Taken because it is the one whose equality with the
// two-launch route needs no argument about the MFMA's internal products, and it keeps every LDS read of the MFMA
// loop as measured for the bf16 kernel; design (b) -- e4m3 fragments converted at read time, scales folded into the
// score and the probability -- saves the extra barrier and the LDS round trip and is the next step if the
// conversion pass shows as the cost (docs/performance.md, "fp8 KV cache", has the measurement).
//   One case is handled apart, and there the two routes differ: a V row below L whose scale is NaN.  In the bf16
//   image its NaN meets P = 0 inside the MFMA and reaches the queries of the tile that the causal mask hides it from;
//   here the row is converted to zeros and the queries that do see it get NaN in the epilogue (convert_tile).
//   Pipeline: the staging image is single and the bf16 image is single; together they are the double buffer.  Per
//   tile: convert staging -> image, barrier, request tile t + 1 into the staging (every wave is past its conversion
//   reads), MFMA work on the image, closing barrier (drains the DMA; the image is free again).  One barrier more per
//   tile than bf16.  LDS at D 128: 2 x 16 KB images + 2 x 8 KB staging + 512 B scales = 48.5 KB (bf16: 64 KB).
#include "fa_common.h"
#include "kernels.h"
#include "kv_cache.h"

namespace bpe {
namespace fa {
namespace cache {

constexpr float RESCALE_THRESHOLD = 8.0f;  // log2 units, as fa_fwd_kernel

// The row scales of a cache format as a kernel argument: nothing for bf16 (an empty last argument, so that
// instantiation's argument layout and code are those of the kernel before it took a format), two pointers for fp8.
template <class C> struct Scales {};
template <> struct Scales<kvc::Fp8Cache> {
    const float* k;
    const float* v;
};

// Dynamic LDS of an instantiation: bf16 K / V [2][64][D] each; fp8 one bf16 image and one byte staging image each,
// then the 64 K and 64 V scales and the first non-finite V row (one int).
template <int D, class C> constexpr size_t lds_bytes() {
    return C::scaled ? (size_t)2 * 64 * D * 2 + 2 * 64 * D + 512 + 16 : (size_t)4 * 64 * D * 2;
}

// 16 staged e4m3 bytes of a row and the row's scale -> the two 16-byte chunks of bf16 that kv_dequant_kernel
// (kv_fp8.hip) writes for them: the same conversions, the same product, the same rounding.
__device__ __forceinline__ void dequant16(u32x4 w, float s, u16x8& lo, u16x8& hi) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const f32x2 a = kvc::fp8x2(w[i], false), c = kvc::fp8x2(w[i], true);
        lo[4 * i] = f2bf(a.x * s); lo[4 * i + 1] = f2bf(a.y * s);
        lo[4 * i + 2] = f2bf(c.x * s); lo[4 * i + 3] = f2bf(c.y * s);
        const f32x2 e = kvc::fp8x2(w[2 + i], false), g = kvc::fp8x2(w[2 + i], true);
        hi[4 * i] = f2bf(e.x * s); hi[4 * i + 1] = f2bf(e.y * s);
        hi[4 * i + 2] = f2bf(g.x * s); hi[4 * i + 3] = f2bf(g.y * s);
    }
}

// The conversion pass of one operand: staging [64][D] bytes + scales [64] -> the swizzled bf16 image swz<2 * D>.
// Thread tid takes the 16-byte pieces tid, tid + 256, ...: lane-linear 16-byte reads, and the 8 lanes of a
// ds_write_b128 group write 8 distinct 16-byte slots of one 256-byte bank row (two 128-byte rows that share sigma at
// D 64, one 256-byte row at D 128; the chunks 2 j ^ sigma of a row all have the parity of sigma).
// `vbad` (V only, else null): a V row whose scale is not finite -- a non-finite row of the sequence itself -- is
// written as zeros and its key index (n0 + row) is min-ed into *vbad instead: inside the MFMA its NaN would reach
// every query of the tile, 0 * NaN, also those the causal mask hides it from.  The epilogue gives NaN to exactly the
// queries that see the row.  (A non-finite K row needs nothing: its scores are masked by a select.)
template <int D>
__device__ __forceinline__ void convert_tile(const char* st, const char* sc, char* img, int tid, int n0 = 0,
                                             int* vbad = nullptr) {
    constexpr int PR = D / 16;  // 16-byte pieces per row
#pragma unroll
    for (int i = 0; i < D / 64; ++i) {
        const int e = tid + 256 * i, r = e / PR, j = e % PR;
        const u32x4 w = *reinterpret_cast<const u32x4*>(st + 16 * e);
        const float s = *reinterpret_cast<const float*>(sc + 4 * r);
        u16x8 lo, hi;
        dequant16(w, s, lo, hi);
        if (vbad != nullptr && !(fabsf(s) < INFINITY)) {
            lo = u16x8{};
            hi = u16x8{};
            if (j == 0) atomicMin(vbad, n0 + r);
        }
        *reinterpret_cast<u16x8*>(img + swz<2 * D>(r, 2 * j)) = lo;
        *reinterpret_cast<u16x8*>(img + swz<2 * D>(r, 2 * j + 1)) = hi;
    }
}

// Requests tile n0 .. n0 + 63 of both operands by LDS-DMA: bf16 into buffer `buf` of the K and of the V pair; fp8
// into the staging images, with the tile's scales (waves 0 and 1, one wave-instruction each).
template <int D, class C> struct Request;

template <int D> struct Request<D, kvc::Bf16Cache> {
    static constexpr int RB = 2 * D, TILE = 64 * RB;
    const __bf16 *kbase, *vbase;
    int sbytes, wu;
    char* smem;
    DmaVoff<4, RB> vo;
    __device__ __forceinline__ Request(const u16* k, const u16* v, int nbytes, char* lds, Scales<kvc::Bf16Cache>,
                                       long, int, int w, int l)
        : kbase((const __bf16*)k), vbase((const __bf16*)v), sbytes(nbytes), wu(w), smem(lds), vo(dma_voff<4, RB>(D, w, l)) {}
    __device__ __forceinline__ void operator()(int n0, int buf) const {
        dma_tile64_buf<4, RB>(kbase, sbytes, vo, n0, D, smem + buf * TILE, wu);
        dma_tile64_buf<4, RB>(vbase, sbytes, vo, n0, D, smem + (2 + buf) * TILE, wu);
    }
};

template <int D> struct Request<D, kvc::Fp8Cache> {
    static constexpr int TILE = 64 * 2 * D;
    const unsigned char *kbase, *vbase;
    const float *ks, *vs;  // the slab's scales
    int sbytes, scbytes, wu, l;
    char* st;  // K staging; V staging, K scales and V scales follow
    __device__ __forceinline__ Request(const unsigned char* k, const unsigned char* v, int nbytes, char* lds,
                                       Scales<kvc::Fp8Cache> sc, long row0, int nsc, int w, int lane)
        : kbase(k), vbase(v), ks(sc.k + row0), vs(sc.v + row0), sbytes(nbytes), scbytes(nsc), wu(w), l(lane),
          st(lds + 2 * TILE) {}
    __device__ __forceinline__ void operator()(int n0, int) const {
        dma_bytes64_buf<4, D>(kbase, sbytes, n0, st, wu, l);
        dma_bytes64_buf<4, D>(vbase, sbytes, n0, st + TILE / 2, wu, l);
        if (wu == 0) dma_scales64_buf(ks, scbytes, n0, st + TILE, l);
        if (wu == 1) dma_scales64_buf(vs, scbytes, n0, st + TILE + 256, l);
    }
};

// The same requests over the paged cache (kv_cache.h PagedLayout; Kc / Vc / scales are the pools).  Tile t lies in
// page t / 4 of the sequence: the resources start at that page's (page, hk) block of KV_PAGE rows, the tile's offset
// inside it is (t % 4) * 64 rows, and the extent is min(KV_PAGE, L - KV_PAGE (t / 4)) rows, so rows from L on still
// read as zeros, bytes and scales.  `pg` is the page id, read by the kernel once per page (wave-uniform, clamped).
template <int D, class C> struct PagedRequest;

template <int D> struct PagedRequest<D, kvc::Bf16Cache> {
    static constexpr int RB = 2 * D, TILE = 64 * RB;
    const __bf16 *k, *v;
    int hk, Hkv, L, wu;
    char* smem;
    DmaVoff<4, RB> vo;
    __device__ __forceinline__ PagedRequest(const u16* kp, const u16* vp, int hk_, int Hkv_, int L_, char* lds,
                                            Scales<kvc::Bf16Cache>, int w, int l)
        : k((const __bf16*)kp), v((const __bf16*)vp), hk(hk_), Hkv(Hkv_), L(L_), wu(w), smem(lds),
          vo(dma_voff<4, RB>(D, w, l)) {}
    __device__ __forceinline__ void operator()(int n0, int buf, int pg) const {
        const long off = ((long)pg * Hkv + hk) * kvc::KV_PAGE * D;
        const int nbytes = min(kvc::KV_PAGE, L - n0 / kvc::KV_PAGE * kvc::KV_PAGE) * RB;
        dma_tile64_buf<4, RB>(k + off, nbytes, vo, n0 % kvc::KV_PAGE, D, smem + buf * TILE, wu);
        dma_tile64_buf<4, RB>(v + off, nbytes, vo, n0 % kvc::KV_PAGE, D, smem + (2 + buf) * TILE, wu);
    }
};

template <int D> struct PagedRequest<D, kvc::Fp8Cache> {
    static constexpr int TILE = 64 * 2 * D;
    const unsigned char *k, *v;
    const float *ks, *vs;  // the pools' scales
    int hk, Hkv, L, wu, l;
    char* st;
    __device__ __forceinline__ PagedRequest(const unsigned char* kp, const unsigned char* vp, int hk_, int Hkv_, int L_,
                                            char* lds, Scales<kvc::Fp8Cache> sc, int w, int lane)
        : k(kp), v(vp), ks(sc.k), vs(sc.v), hk(hk_), Hkv(Hkv_), L(L_), wu(w), l(lane), st(lds + 2 * TILE) {}
    __device__ __forceinline__ void operator()(int n0, int, int pg) const {
        const long row0 = ((long)pg * Hkv + hk) * kvc::KV_PAGE;
        const int rows = min(kvc::KV_PAGE, L - n0 / kvc::KV_PAGE * kvc::KV_PAGE), r0 = n0 % kvc::KV_PAGE;
        dma_bytes64_buf<4, D>(k + row0 * D, rows * D, r0, st, wu, l);
        dma_bytes64_buf<4, D>(v + row0 * D, rows * D, r0, st + TILE / 2, wu, l);
        if (wu == 0) dma_scales64_buf(ks + row0, rows * 4, r0, st + TILE, l);
        if (wu == 1) dma_scales64_buf(vs + row0, rows * 4, r0, st + TILE + 256, l);
    }
};

// The packed form's work (kv_cache.h PackedMap; cache_attn_packed): workgroup blockIdx.x is kv head blockIdx.x % Hkv of
// item blockIdx.x / Hkv of a host-built list `work [W, 2]` of (sequence, 128-row query block), heaviest first.  A
// sequence's blocks count from its own row 0, so a block never straddles two sequences and everything a workgroup
// computes -- q0, p0, L, the limits, ntiles -- is what the uniform kernel computes for that slot alone with T = n: the
// same bits.  The table and the list are device data like pos: every value read from them is clamped into range, so
// no content of either addresses outside q / o (N rows) or the cache.
struct PackedWork {
    static constexpr bool packed = true;
    kvc::PackedMap map;
    const int* work;
    int N;
};

// Lay (kv_cache.h): the cache layout.  The slab instantiations take an empty `lay` and are the code they were.
// Map: kvc::UniformMap (B sequences of Tu tokens, workgroups from blockIdx and nqb; an empty `map`) or PackedWork
// (Tu, nqb and pstride are not read).
template <int D, class C, class Lay = kvc::SlabLayout, class Map = kvc::UniformMap>
__global__ void __launch_bounds__(256, 2)
cache_attn_kernel(const __bf16* __restrict__ Q, const typename C::elem* __restrict__ Kc,
                  const typename C::elem* __restrict__ Vc, __bf16* __restrict__ O, const int* __restrict__ pos,
                  int pstride, int H, int Hkv, int Lmax, int Tu, float scale_log2, int nqb, Scales<C> sc, Lay lay,
                  Map map) {
    constexpr int RB = D * 2;      // bytes per LDS row
    constexpr int TILE = 64 * RB;  // bytes per 64-key tile
    constexpr int KS = D / 16;     // k-steps over the head dim
    constexpr int DT = D / 32;     // 32-wide d tiles of O
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* Ks = smem;                                // bf16 [2][64][D]; fp8: the K image, then the V image
    char* Vs = smem + (C::scaled ? 1 : 2) * TILE;   // bf16 [2][64][D]
    char* Kst = smem + 2 * TILE;                    // fp8: staged bytes [64][D] of K, of V, then the scales
    char* Vst = Kst + TILE / 2;
    char* Ksc = Vst + TILE / 2;
    char* Vsc = Ksc + 256;
    int* vbad = reinterpret_cast<int*>(Vsc + 256);  // fp8: the first V row with a non-finite scale

    const int tid = threadIdx.x, w = tid >> 6, l = tid & 63, l31 = l & 31, hh = l >> 5;
    const int wu = __builtin_amdgcn_readfirstlane(w);
    int bk, qb, b, hk, T;
    [[maybe_unused]] int qoff = 0;  // packed: first row of the sequence in Q / O
    if constexpr (Map::packed) {
        const int item = (int)blockIdx.x / Hkv;
        hk = (int)blockIdx.x % Hkv;
        const int i = min(max(map.work[2 * item], 0), map.map.S - 1);
        qb = max(map.work[2 * item + 1], 0);
        b = map.map.slot(i);
        T = min(max(map.map.n(i), 1), map.N);
        qoff = min(max(map.map.off(i), 0), map.N - T);
        bk = b * Hkv + hk;
    } else {
        const int BK = (int)gridDim.x / nqb;
        bk = (int)blockIdx.x % BK;               // b * Hkv + hk
        qb = nqb - 1 - (int)blockIdx.x / BK;     // heaviest (last) row blocks first
        b = bk / Hkv, hk = bk % Hkv;
        T = Tu;
    }
    // row of token `tok` of this sequence in Q / O
    const auto qo_row = [&](int tok) -> long {
        if constexpr (Map::packed) return (long)qoff + tok;
        else return (long)b * T + tok;
    };
    const int G = H / Hkv, R = G * T;
    // any int32 contents of pos give in-range tiles: 0 <= p0 <= Lmax, 1 <= L <= Lmax
    const int p0 = min(max(pos[Map::packed ? b : b * pstride], 0), Lmax);
    const int L = min(p0 + T, Lmax);  // rows of the slab that hold this sequence's keys
    const int q0 = qb * 128, qw0 = q0 + 32 * wu;
    const int qrow = qw0 + l31;
    const int rq = min(qrow, R - 1);  // rows past the end clamped (computed, not stored)
    const int tok = rq / G, head = hk * G + rq % G;
    const int lim = min(p0 + tok, L - 1);  // the lane's last visible key

    // the Q rows and K / V tile 0 are requested before any is waited for
    u16x8 qr[KS];
    {
        const __bf16* qp = Q + (qo_row(tok) * H + head) * D;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) qr[ks] = *reinterpret_cast<const u16x8*>(qp + 16 * ks + 8 * hh);
    }
    // wave-uniform limits: of the wave's first and last row, and of the block's last row
    const bool wave_on = qw0 < R;
    const int lim_lo = min(p0 + min(qw0, R - 1) / G, L - 1);
    const int lim_hi = min(p0 + min(qw0 + 31, R - 1) / G, L - 1);
    const int ntiles = (min(p0 + min(q0 + 127, R - 1) / G, L - 1) + 64) / 64;  // >= 1

    const typename C::elem* kbase = Kc + (long)bk * Lmax * D;
    const typename C::elem* vbase = Vc + (long)bk * Lmax * D;
    const int sbytes = L * D * (int)sizeof(typename C::elem);  // extent of both resources: rows >= L read as zeros
    if constexpr (C::scaled) {
        if (tid == 0) *vbad = 0x7fffffff;
    }
    // paged: the page id of the tile being requested, read from the table when a request enters a new page (n0 <= L - 1
    // < Lmax <= NB * KV_PAGE, so the entry exists; wave-uniform: b and n0 are)
    [[maybe_unused]] int pg = 0;
    const auto make_request = [&] {
        if constexpr (Lay::paged) return PagedRequest<D, C>{Kc, Vc, hk, Hkv, L, smem, sc, wu, l};
        else return Request<D, C>{kbase, vbase, sbytes, smem, sc, (long)bk * Lmax, L * 4, wu, l};
    };
    const auto req = make_request();
    const auto request = [&](int n0, int buf) {
        if constexpr (Lay::paged) {
            if (n0 % kvc::KV_PAGE == 0) pg = __builtin_amdgcn_readfirstlane(lay.page_clamped(b, n0 / kvc::KV_PAGE));
            req(n0, buf, pg);
        } else {
            req(n0, buf);
        }
    };
    request(0, 0);

    // Q fragments (B operand of S^T = K.Q^T), softmax scale * log2(e) folded in
    bf16x8 qf[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
        float x[8];
        unpack8(qr[ks], x);
        qf[ks] = __builtin_bit_cast(bf16x8, pack8(x, scale_log2));
    }

    f32x16 o[DT];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[dt][r] = 0.f;
    float m_run = -INFINITY, l_run = 0.f;

    const int trow = 4 * hh + ((l & 15) >> 2);           // tr-read row inside a 16-key step
    const int tcol = 16 * ((l >> 4) & 1) + 4 * (l & 3);  // tr-read column inside a 32-wide d tile

    __syncthreads();
    for (int t = 0; t < ntiles; ++t) {
        const int cur = C::scaled ? 0 : t & 1, n0 = t * 64;
        if constexpr (!C::scaled) {
            // buffer cur ^ 1 was last read in tile t - 1, before its closing barrier
            if (t + 1 < ntiles) request(n0 + 64, cur ^ 1);
        } else {
            // every wave converts, whether it has work in this tile or not.  The images were last read in tile
            // t - 1, before its closing barrier, which also drained this tile's DMA; the staging is requested again
            // only after the barrier below, when no wave reads it any more.
            convert_tile<D>(Kst, Ksc, Ks, tid);
            convert_tile<D>(Vst, Vsc, Vs, tid, n0, vbad);
            __syncthreads();
            if (t + 1 < ntiles) request(n0 + 64, 0);
        }
        if (wave_on && n0 <= lim_hi) {
            const char* Kt = Ks + cur * TILE;
            char* Vt = Vs + cur * TILE;
            f32x16 s[2];
#pragma unroll
            for (int kt = 0; kt < 2; ++kt) {
#pragma unroll
                for (int r = 0; r < 16; ++r) s[kt][r] = 0.f;
#pragma unroll
                for (int ks = 0; ks < KS; ++ks)
                    s[kt] = mfma(lds_row16(Kt, swz<RB>(kt * 32 + l31, 2 * ks + hh)), qf[ks], s[kt]);
            }
            if (n0 + 63 > lim_lo) {  // diagonal or tail tile (wave-uniform; lim_lo <= L - 1 covers the tail)
                // key n0 + 32 kt + acc_row(r, hh) is visible iff it is <= lim: one compare of the lane's limit
                // against the register's compile-time row offset and one select per score
                const int qlim = lim - n0 - 4 * hh;
#pragma unroll
                for (int kt = 0; kt < 2; ++kt)
#pragma unroll
                    for (int r = 0; r < 16; ++r)
                        if ((r & 3) + 8 * (r >> 2) > qlim - 32 * kt) s[kt][r] = -INFINITY;
            }
            float mt = s[0][0];
#pragma unroll
            for (int kt = 0; kt < 2; ++kt)
#pragma unroll
                for (int r = 0; r < 16; ++r) mt = fmaxf(mt, s[kt][r]);
            mt = fmaxf(mt, __shfl_xor(mt, 32, 64));
            // deferred rescale: the running max moves only when this tile exceeds it by more than the threshold
            const bool grow = mt > m_run + RESCALE_THRESHOLD;
            float alpha = 1.f;
            if (grow) {
                alpha = fast_exp2(m_run - mt);  // m_run = -inf on the first tile -> 0
                m_run = mt;
            }
            const float mu = (m_run == -INFINITY) ? 0.f : m_run;
            float ls = 0.f;
#pragma unroll
            for (int kt = 0; kt < 2; ++kt)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float p = fast_exp2(s[kt][r] - mu);
                    s[kt][r] = p;
                    ls += p;
                }
            ls += __shfl_xor(ls, 32, 64);
            l_run = l_run * alpha + ls;
            if (!__all(!grow)) {
#pragma unroll
                for (int dt = 0; dt < DT; ++dt)
#pragma unroll
                    for (int r = 0; r < 16; ++r) o[dt][r] *= alpha;
            }
            // P^T fragments: k-step kk = (key tile kt, half ss) in the accumulator's permuted k order
            bf16x8 pf[4];
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
                const int kt = kk >> 1, ss = kk & 1;
#pragma unroll
                for (int j = 0; j < 8; ++j) pf[kk][j] = (__bf16)s[kt][8 * ss + j];
            }
#pragma unroll
            for (int dt = 0; dt < DT; ++dt)
#pragma unroll
                for (int kk = 0; kk < 4; ++kk) {
                    const int kb = (kk >> 1) * 32 + 16 * (kk & 1);
                    const bf16x8 va = lds_tr_pair(Vt, tr_off<RB>(kb + trow, dt * 32 + tcol),
                                                  tr_off<RB>(kb + 8 + trow, dt * 32 + tcol));
                    o[dt] = mfma(va, pf[kk], o[dt]);
                }
        }
        // no barrier after the last tile: a wave done with it does not wait for the others
        if (t + 1 < ntiles) __syncthreads();
    }

    // ---- epilogue: O = O^T / l, query on the lane, 4 consecutive d per register group
    if (qrow < R) {
        float inv = l_run > 0.f ? 1.f / l_run : 0.f;
        if constexpr (C::scaled) {
            // a visible non-finite V row: the whole output row is NaN, as p * NaN gives for every d (the last
            // conversion pass, and with it the last atomicMin, lies before a barrier this wave has passed)
            if (*vbad <= lim) inv = __uint_as_float(0x7fc00000u);
        }
        __bf16* op = O + (qo_row(tok) * H + head) * D;
#pragma unroll
        for (int dt = 0; dt < DT; ++dt)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const u16x4 v = {f2bf(o[dt][4 * i] * inv), f2bf(o[dt][4 * i + 1] * inv),
                                 f2bf(o[dt][4 * i + 2] * inv), f2bf(o[dt][4 * i + 3] * inv)};
                *reinterpret_cast<u16x4*>(op + dt * 32 + 8 * i + 4 * hh) = v;
            }
    }
}

}  // namespace cache
}  // namespace fa
}  // namespace bpe

using namespace bpe;
using namespace bpe::fa;

// T new tokens per sequence over the cache: any T, the G heads of a kv head share a workgroup's rows.  The slab
// extent (Lmax rows of D bf16) is a 32-bit byte count of the buffer resources.
static bool cache_shape_ok(int H, int Hkv, int D, int T, int Lmax) {
    const int G = Hkv > 0 ? H / Hkv : 0;
    return (D == 64 || D == 128) && Hkv > 0 && H % Hkv == 0 && G >= 1 && G <= 8 && T >= 1 && Lmax >= 1 &&
           (long)G * T < (1L << 30);
}

bool cache_attn_ok(int H, int Hkv, int D, int T, int Lmax) {
    return cache_shape_ok(H, Hkv, D, T, Lmax) && (long)Lmax * D * 2 < (1L << 31);
}

// (A paged cache's extents are those of one page, 256 rows: the slab bounds, which a pool always meets, still apply
// to Lmax as the range of the row indices.)
// The e4m3 cache: the 32-bit extents are Lmax * D bytes of a slab and Lmax * 4 bytes of its scales.
bool cache_attn_fp8_ok(int H, int Hkv, int D, int T, int Lmax) {
    return cache_shape_ok(H, Hkv, D, T, Lmax) && (long)Lmax * D < (1L << 31) && (long)Lmax * 4 < (1L << 31);
}

template <int D, class C, class Lay>
static void cache_launch_lay(const void* q, const void* k, const void* v, cache::Scales<C> sc, void* out,
                             const int* pos, int pstride, int B, int T, int H, int Hkv, int Lmax, float scale, Lay lay,
                             hipStream_t s) {
    typedef const typename C::elem* cptr;
    const int nqb = ((H / Hkv) * T + 127) / 128;
    cache::cache_attn_kernel<D, C, Lay><<<nqb * B * Hkv, 256, cache::lds_bytes<D, C>(), s>>>(
        (const __bf16*)q, (cptr)k, (cptr)v, (__bf16*)out, pos, pstride, H, Hkv, Lmax, T, scale * LOG2E, nqb, sc, lay,
        kvc::UniformMap{});
}

// The packed form: one workgroup per (work item, kv head), in the list's order (the host sorts it heaviest first).
template <int D, class C>
static void cache_launch_packed(const void* q, const void* k, const void* v, cache::Scales<C> sc, void* out,
                                const int* pos, const KvPacked& pk, int B, int H, int Hkv, int Lmax, float scale,
                                const KvPages& pg, hipStream_t s) {
    typedef const typename C::elem* cptr;
    const cache::PackedWork map{kvc::PackedMap{pk.seq, pk.S, B}, pk.work, pk.N};
    const int grid = pk.W * Hkv;
    if (pg.table != nullptr)
        cache::cache_attn_kernel<D, C, kvc::PagedLayout, cache::PackedWork>
            <<<grid, 256, cache::lds_bytes<D, C>(), s>>>((const __bf16*)q, (cptr)k, (cptr)v, (__bf16*)out, pos, 1, H,
                                                         Hkv, Lmax, 0, scale * LOG2E, 0, sc,
                                                         kvc::PagedLayout{pg.table, pg.NB, pg.P}, map);
    else
        cache::cache_attn_kernel<D, C, kvc::SlabLayout, cache::PackedWork>
            <<<grid, 256, cache::lds_bytes<D, C>(), s>>>((const __bf16*)q, (cptr)k, (cptr)v, (__bf16*)out, pos, 1, H,
                                                         Hkv, Lmax, 0, scale * LOG2E, 0, sc, kvc::SlabLayout{}, map);
}

template <int D, class C>
static void cache_launch(const void* q, const void* k, const void* v, cache::Scales<C> sc, void* out, const int* pos,
                         int pstride, int B, int T, int H, int Hkv, int Lmax, float scale, const KvPages& pg,
                         hipStream_t s) {
    if (pg.table != nullptr)
        cache_launch_lay<D, C>(q, k, v, sc, out, pos, pstride, B, T, H, Hkv, Lmax, scale,
                               kvc::PagedLayout{pg.table, pg.NB, pg.P}, s);
    else cache_launch_lay<D, C>(q, k, v, sc, out, pos, pstride, B, T, H, Hkv, Lmax, scale, kvc::SlabLayout{}, s);
}

void launch_cache_attn(const void* q, const void* k, const void* v, void* out, const int* pos, int pos_stride, int B,
                       int T, int H, int Hkv, int D, int Lmax, float scale, hipStream_t s, const KvPages& pg) {
    const cache::Scales<kvc::Bf16Cache> none{};
    if (D == 64) cache_launch<64, kvc::Bf16Cache>(q, k, v, none, out, pos, pos_stride, B, T, H, Hkv, Lmax, scale, pg, s);
    else cache_launch<128, kvc::Bf16Cache>(q, k, v, none, out, pos, pos_stride, B, T, H, Hkv, Lmax, scale, pg, s);
}

void launch_cache_attn_fp8(const void* q, const void* k8, const void* v8, const float* ks, const float* vs, void* out,
                           const int* pos, int pos_stride, int B, int T, int H, int Hkv, int D, int Lmax, float scale,
                           hipStream_t s, const KvPages& pg) {
    const cache::Scales<kvc::Fp8Cache> sc{ks, vs};
    if (D == 64) cache_launch<64, kvc::Fp8Cache>(q, k8, v8, sc, out, pos, pos_stride, B, T, H, Hkv, Lmax, scale, pg, s);
    else cache_launch<128, kvc::Fp8Cache>(q, k8, v8, sc, out, pos, pos_stride, B, T, H, Hkv, Lmax, scale, pg, s);
}

void launch_cache_attn_packed(const void* q, const void* k, const void* v, void* out, const int* pos,
                              const KvPacked& pk, int B, int H, int Hkv, int D, int Lmax, float scale, hipStream_t s,
                              const KvPages& pg) {
    const cache::Scales<kvc::Bf16Cache> none{};
    if (D == 64) cache_launch_packed<64, kvc::Bf16Cache>(q, k, v, none, out, pos, pk, B, H, Hkv, Lmax, scale, pg, s);
    else cache_launch_packed<128, kvc::Bf16Cache>(q, k, v, none, out, pos, pk, B, H, Hkv, Lmax, scale, pg, s);
}

void launch_cache_attn_packed_fp8(const void* q, const void* k8, const void* v8, const float* ks, const float* vs,
                                  void* out, const int* pos, const KvPacked& pk, int B, int H, int Hkv, int D, int Lmax,
                                  float scale, hipStream_t s, const KvPages& pg) {
    const cache::Scales<kvc::Fp8Cache> sc{ks, vs};
    if (D == 64) cache_launch_packed<64, kvc::Fp8Cache>(q, k8, v8, sc, out, pos, pk, B, H, Hkv, Lmax, scale, pg, s);
    else cache_launch_packed<128, kvc::Fp8Cache>(q, k8, v8, sc, out, pos, pk, B, H, Hkv, Lmax, scale, pg, s);
}
