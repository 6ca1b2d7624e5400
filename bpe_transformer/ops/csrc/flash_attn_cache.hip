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
#include "fa_common.h"
#include "kernels.h"

namespace bpe {
namespace fa {
namespace cache {

constexpr float RESCALE_THRESHOLD = 8.0f;  // log2 units, as fa_fwd_kernel

template <int D>
__global__ void __launch_bounds__(256, 2)
cache_attn_kernel(const __bf16* __restrict__ Q, const __bf16* __restrict__ Kc, const __bf16* __restrict__ Vc,
                  __bf16* __restrict__ O, const int* __restrict__ pos, int pstride, int H, int Hkv, int Lmax, int T,
                  float scale_log2, int nqb) {
    constexpr int RB = D * 2;      // bytes per LDS row
    constexpr int TILE = 64 * RB;  // bytes per 64-key tile
    constexpr int KS = D / 16;     // k-steps over the head dim
    constexpr int DT = D / 32;     // 32-wide d tiles of O
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* Ks = smem;             // [2][64][D]
    char* Vs = smem + 2 * TILE;  // [2][64][D]

    const int tid = threadIdx.x, w = tid >> 6, l = tid & 63, l31 = l & 31, hh = l >> 5;
    const int wu = __builtin_amdgcn_readfirstlane(w);
    const int BK = (int)gridDim.x / nqb;
    const int bk = (int)blockIdx.x % BK;               // b * Hkv + hk
    const int qb = nqb - 1 - (int)blockIdx.x / BK;     // heaviest (last) row blocks first
    const int b = bk / Hkv, hk = bk % Hkv;
    const int G = H / Hkv, R = G * T;
    // any int32 contents of pos give in-range tiles: 0 <= p0 <= Lmax, 1 <= L <= Lmax
    const int p0 = min(max(pos[b * pstride], 0), Lmax);
    const int L = min(p0 + T, Lmax);  // rows of the slab that hold this sequence's keys
    const int q0 = qb * 128, qw0 = q0 + 32 * wu;
    const int qrow = qw0 + l31;
    const int rq = min(qrow, R - 1);  // rows past the end clamped (computed, not stored)
    const int tok = rq / G, head = hk * G + rq % G;
    const int lim = min(p0 + tok, L - 1);  // the lane's last visible key

    // the Q rows and K / V tile 0 are requested before any is waited for
    u16x8 qr[KS];
    {
        const __bf16* qp = Q + (((long)b * T + tok) * H + head) * D;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) qr[ks] = *reinterpret_cast<const u16x8*>(qp + 16 * ks + 8 * hh);
    }
    // wave-uniform limits: of the wave's first and last row, and of the block's last row
    const bool wave_on = qw0 < R;
    const int lim_lo = min(p0 + min(qw0, R - 1) / G, L - 1);
    const int lim_hi = min(p0 + min(qw0 + 31, R - 1) / G, L - 1);
    const int ntiles = (min(p0 + min(q0 + 127, R - 1) / G, L - 1) + 64) / 64;  // >= 1

    const __bf16* kbase = Kc + (long)bk * Lmax * D;
    const __bf16* vbase = Vc + (long)bk * Lmax * D;
    const int sbytes = L * D * 2;  // extent of both buffer resources: rows >= L read as zeros
    const DmaVoff<4, RB> vo = dma_voff<4, RB>(D, wu, l);
    dma_tile64_buf<4, RB>(kbase, sbytes, vo, 0, D, Ks, wu);
    dma_tile64_buf<4, RB>(vbase, sbytes, vo, 0, D, Vs, wu);

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
        const int cur = t & 1, n0 = t * 64;
        if (t + 1 < ntiles) {  // buffer cur ^ 1 was last read in tile t - 1, before its closing barrier
            dma_tile64_buf<4, RB>(kbase, sbytes, vo, n0 + 64, D, Ks + (cur ^ 1) * TILE, wu);
            dma_tile64_buf<4, RB>(vbase, sbytes, vo, n0 + 64, D, Vs + (cur ^ 1) * TILE, wu);
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
        const float inv = l_run > 0.f ? 1.f / l_run : 0.f;
        __bf16* op = O + (((long)b * T + tok) * H + head) * D;
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
bool cache_attn_ok(int H, int Hkv, int D, int T, int Lmax) {
    const int G = Hkv > 0 ? H / Hkv : 0;
    return (D == 64 || D == 128) && Hkv > 0 && H % Hkv == 0 && G >= 1 && G <= 8 && T >= 1 && Lmax >= 1 &&
           (long)Lmax * D * 2 < (1L << 31) && (long)G * T < (1L << 30);
}

template <int D>
static void cache_launch(const void* q, const void* k, const void* v, void* out, const int* pos, int pstride, int B,
                         int T, int H, int Hkv, int Lmax, float scale, hipStream_t s) {
    const int nqb = ((H / Hkv) * T + 127) / 128;
    cache::cache_attn_kernel<D><<<nqb * B * Hkv, 256, (size_t)4 * 64 * D * 2, s>>>(
        (const __bf16*)q, (const __bf16*)k, (const __bf16*)v, (__bf16*)out, pos, pstride, H, Hkv, Lmax, T,
        scale * LOG2E, nqb);
}

void launch_cache_attn(const void* q, const void* k, const void* v, void* out, const int* pos, int pos_stride, int B,
                       int T, int H, int Hkv, int D, int Lmax, float scale, hipStream_t s) {
    if (D == 64) cache_launch<64>(q, k, v, out, pos, pos_stride, B, T, H, Hkv, Lmax, scale, s);
    else cache_launch<128>(q, k, v, out, pos, pos_stride, B, T, H, Hkv, Lmax, scale, s);
}
