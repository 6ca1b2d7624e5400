// KV-cache decode attention and KV-cache append, gfx950.  Serving path of the framework: the reference has no
// inference engine (SURVEY §1 "absent layers"); generation with a KV cache reuses the training model's weights
// (`models/generation.py`).
//
//   q [B, H, D] (RoPE already applied), cache K / V [B, Hkv, Lmax, D] (roped K), valid length L = *pos + 1:
//   out[b, h] = softmax(q . K[b, h / G, :L]^T * scale) . V[b, h / G, :L]          (G = H / Hkv)
// (T > 1 new tokens per sequence, G * T <= 8 -- speculative verification -- is the same with one query row per
// (token, head) and token t limited to L = *pos + t + 1.  Longer windows -- a second turn, chunked prefill into a
// filled cache -- run on the MFMA kernel of flash_attn_cache.hip.)
//
// The position lives in device memory (int32), so one decode step -- append + attention for every layer -- is
// shape-static and is captured once into a HIP graph (the host never passes the growing length).
//
// Memory-bound (one pass over K and V per token), so the design is about bandwidth, not MFMA (guide
// Appendix B "Attention decode": K/V straight to VGPRs): the key range is split into chunks of CH keys, one
// workgroup per (batch, kv head, chunk) handles all G query heads of that kv head, so K and V are read once
// for the G heads.
//   1. scores: thread t owns key t of the chunk, streams its K row (16-byte loads) and dots it with the G query
//      rows (fp32, broadcast from LDS);
//   2. per head: block max / sum of exp over the chunk (fp32);
//   3. o[g][d] = sum_t p[g][t] V[t][d]: thread = (key partition, 8-wide d vector), 16-byte V loads; partitions
//      are reduced inside the wave with lane shuffles, then across the 4 waves through LDS;
//   4. the partial (o, m, l) of every (b, h, chunk) goes to fp32 scratch; a combine kernel merges the chunks
//      (flash-decoding) and writes bf16.  Chunks past the valid length write m = -inf and are skipped.  The
//      small-batch decode step skips the combine launch: the output projection's prologue merges the partials
//      (decode_gemv.hip, GemvArgs::part).
// All of a chunk's K and V loads are issued at kernel entry (register-resident, <= 128 VGPRs at D = 128).
//
// One kernel body serves both cache formats (kv_cache.h): the bf16 cache above, and the fp8 cache of kv_fp8.hip, e4m3
// rows k8 / v8 [B, Hkv, Lmax, D] with one power-of-two fp32 scale each, ks / vs [B, Hkv, Lmax] -- half the bytes
// per key: a thread loads its key's D bytes in D / 16 16-byte loads plus one scale, and 8 bytes per (key, 8-wide d)
// of V.  k_scale[t] multiplies the score, v_scale[t] the probability p[r][t] (the row sum l takes the unscaled p).
// Chunking, the empty-chunk rule, the partials layout and the combine do not depend on the format
// (decode_combine_kernel and decode_attn_proj consume the partials of either).
//
// kv_append_kernel writes the bf16 cache; its fp8 counterpart (kv_fp8.hip) shares the index / RoPE prologue
// (kv_cache.h, append_vec), so both return the same q.
//
// Resources (hipcc -O3, gfx950, -Rpass-analysis=kernel-resource-usage), scratch 0 in every kernel; MR 1 / 2 / 4 / 8:
//   decode_attn_kernel<64, MR, Bf16Cache>   VGPRs 90 / 107 / 122 / 180   SGPRs 47 / 51 / 51 / 56   waves/SIMD 5 / 4 / 4 / 2
//   decode_attn_kernel<128, MR, Bf16Cache>  VGPRs 154 / 168 / 200 / 242  SGPRs 61 / 67 / 72 / 66   waves/SIMD 3 / 3 / 2 / 2
//   decode_attn_kernel<64, MR, Fp8Cache>    VGPRs 62 / 80 / 96 / 180     SGPRs 47 / 51 / 51 / 56   waves/SIMD 8 / 6 / 5 / 2
//   decode_attn_kernel<128, MR, Fp8Cache>   VGPRs 94 / 112 / 120 / 180   SGPRs 61 / 67 / 72 / 66   waves/SIMD 5 / 4 / 4 / 2
//   LDS bytes, either format: D 64: 2336 / 4640 / 9248 / 18464, D 128: 3616 / 7200 / 14368 / 28704
//   kv_append_kernel VGPRs 44, SGPRs 69   kv_append_fp8_kernel VGPRs 44, SGPRs 79   kv_dequant_kernel VGPRs 29   (8 waves)
//   cache_attn_kernel<64 / 128, Bf16Cache>  VGPRs 118 / 176   SGPRs 41 / 41   LDS 32768 / 65536   waves/SIMD 4 / 2
//   cache_attn_kernel<64 / 128, Fp8Cache>   VGPRs 122 / 184   SGPRs 52 / 54   LDS 25104 / 49680   waves/SIMD 4 / 2
//     (flash_attn_cache.hip)
// The format's scale loads and multiplies exist only in the Fp8Cache instantiations (`if constexpr`).
// Paged layout (kv_cache.h PagedLayout; the rows above are the SlabLayout instantiations, unchanged by it).  LDS and
// scratch as the slab twin; no paged instantiation loses a wave per SIMD against its twin:
//   decode_attn_kernel<64, MR, Bf16Cache, PagedLayout>   VGPRs 90 / 107 / 122 / 180   SGPRs 48 / 51 / 51 / 56   waves/SIMD 5 / 4 / 4 / 2
//   decode_attn_kernel<128, MR, Bf16Cache, PagedLayout>  VGPRs 154 / 168 / 200 / 242  SGPRs 64 / 67 / 72 / 67   waves/SIMD 3 / 3 / 2 / 2
//   decode_attn_kernel<64, MR, Fp8Cache, PagedLayout>    VGPRs 60 / 80 / 96 / 180     SGPRs 48 / 51 / 51 / 56   waves/SIMD 8 / 6 / 5 / 2
//   decode_attn_kernel<128, MR, Fp8Cache, PagedLayout>   VGPRs 92 / 110 / 118 / 180   SGPRs 64 / 67 / 72 / 67   waves/SIMD 5 / 4 / 4 / 2
//   kv_append_kernel<PagedLayout> VGPRs 42, SGPRs 72   kv_append_fp8_kernel<PagedLayout> VGPRs 42, SGPRs 83   (8 waves)
//   cache_attn_kernel<64 / 128, Bf16Cache, PagedLayout>  VGPRs 118 / 176   SGPRs 48 / 47   waves/SIMD 4 / 2
//   cache_attn_kernel<64 / 128, Fp8Cache, PagedLayout>   VGPRs 122 / 184   SGPRs 60 / 62   waves/SIMD 4 / 2
// Packed map (kv_cache.h PackedMap / flash_attn_cache.hip PackedWork: the prompts of several slots in one launch).  One
// body serves both maps; the rows above are the UniformMap instantiations, unchanged by it (cache_attn_kernel<., Bf16Cache>
// on slabs went from 43 to 41 SGPRs).  The packed instantiations, slab / paged, LDS as the uniform twin, scratch 0:
//   kv_append_kernel<., PackedMap>      VGPRs 42 / 40   SGPRs 69 / 72   kv_append_fp8_kernel<., PackedMap>  VGPRs 42 / 40
//                                       SGPRs 81 / 84   (8 waves)
//   cache_attn_kernel<64 / 128, Bf16Cache, SlabLayout, PackedWork>   VGPRs 118 / 176   SGPRs 40 / 40   waves/SIMD 4 / 2
//   cache_attn_kernel<64 / 128, Bf16Cache, PagedLayout, PackedWork>  VGPRs 118 / 176   SGPRs 48 / 47   waves/SIMD 4 / 2
//   cache_attn_kernel<64 / 128, Fp8Cache, SlabLayout, PackedWork>    VGPRs 122 / 184   SGPRs 52 / 54   waves/SIMD 4 / 2
//   cache_attn_kernel<64 / 128, Fp8Cache, PagedLayout, PackedWork>   VGPRs 122 / 184   SGPRs 60 / 62   waves/SIMD 4 / 2
#include "kv_cache.h"
#include "kernels.h"

namespace bpe {
namespace dec {

using namespace kvc;

constexpr int CH = 256;  // keys per chunk (= threads per workgroup)

// MR (query rows per workgroup, >= G * T) is a template parameter: the per-row registers (m, l, o accumulators)
// must be statically indexed (guide §5.4 rule 20: runtime-indexed register arrays go to scratch).  Row r is
// new token t = r / G of the sequence and query head g = r % G of the kv head; with T new tokens at positions
// p0 .. p0 + T - 1 (p0 = *pos, already in the cache), token t attends keys [0, p0 + t] (causal within the chunk).
// Fmt (kv_cache.h) is the cache format; Ks / Vs are read only where it has scales (null otherwise).  Both formats
// run the same floating-point operations in the same order on the unpacked values; a key's scale multiplies its
// finished score, a value's scale its probability, and no bf16 instruction sees either.
// Lay (kv_cache.h) is the cache layout.  Paged: Kc / Vc (Ks / Vs) are the pools, chunk `split` of sequence b is the
// page table[b, split] (clamped into the pool), and everything after `rowbase` is the slab kernel's code.
template <int D, int MR, class Fmt, class Lay = SlabLayout>
__global__ void __launch_bounds__(256) decode_attn_kernel(const __bf16* __restrict__ q, const void* __restrict__ Kc,
                                                          const void* __restrict__ Vc, const float* __restrict__ Ks,
                                                          const float* __restrict__ Vs, float* __restrict__ part,
                                                          const int* __restrict__ pos, int pstride, int H, int Hkv,
                                                          int Lmax, int nsplit, float scale, int T, Lay lay) {
    static_assert(CH == KV_PAGE, "a chunk is one page");
    typedef typename Fmt::elem elem;
    typedef typename Fmt::KVec KVec;
    typedef typename Fmt::VVec VVec;
    constexpr int DV = D / 8;        // 8-element vectors per row
    constexpr int NK = D / Fmt::KE;  // 16-byte registers of a key row
    constexpr int KP = 256 / DV;     // key partitions of the P.V step
    __shared__ float qs[MR][D];
    __shared__ float ps[MR][CH];
    __shared__ float red[2][4];
    __shared__ float ob[4][MR][D];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int bk = blockIdx.x / nsplit, split = blockIdx.x % nsplit;  // bk = b * Hkv + hk
    const int b = bk / Hkv, hk = bk % Hkv;
    const int G = H / Hkv, R = G * T;
    const int p0 = pos[b * pstride];  // pstride 0: one position for the batch, 1: one per sequence (uniform: one b)
    const int L = min(p0 + T, Lmax);  // keys any row of this workgroup may see
    const int s0 = split * CH;
    // partial slot of row r: part[(((b * T + t) * H + h) * nsplit + split) * (D + 2)]
    auto prow = [&](int r) {
        return part + ((((long)b * T + r / G) * H + hk * G + r % G) * nsplit + split) * (D + 2);
    };
    if (s0 >= L) {  // uniform per workgroup: an empty chunk contributes nothing
        if (tid < R) {
            float* pr = prow(tid);
            pr[D] = -INFINITY;
            pr[D + 1] = 0.f;
        }
        return;
    }
    const int n = min(CH, L - s0);
    long rowbase;  // first cache row of the chunk (its scale is at rowbase)
    if constexpr (Lay::paged) rowbase = ((long)lay.page_clamped(b, split) * Hkv + hk) * KV_PAGE;
    else rowbase = (long)bk * Lmax + s0;
    const long kvbase = rowbase * D;            // and its first element
    // every K and V load of the chunk is issued up front (latency-bound at small batch: the q staging, the
    // score reductions and the softmax run while they are in flight): the key's row (and scale), the value scale of
    // key tid (folded into p below), and the V elements of this thread's (key partition, d vector) slots
    const bool ok = tid < n;
    KVec kr[NK];
    {
        const KVec* kp = reinterpret_cast<const KVec*>(Fmt::row(Kc, rowbase, tid, D));
#pragma unroll
        for (int v = 0; v < NK; ++v) kr[v] = ok ? kp[v] : KVec{};
    }
    [[maybe_unused]] float ksc = 0.f, vsc = 0.f;
    if constexpr (Fmt::scaled) {
        ksc = ok ? Ks[rowbase + tid] : 0.f;
        vsc = ok ? Vs[rowbase + tid] : 0.f;
    }
    const int dv = tid % DV, kp = tid / DV;
    VVec vr[CH / KP];
#pragma unroll
    for (int j = 0; j < CH / KP; ++j) {
        const int t = kp + KP * j;
        vr[j] = t < n ? *reinterpret_cast<const VVec*>(Fmt::row(Vc, rowbase, t, D) + dv * 8) : VVec{};
    }
    // query rows -> LDS (fp32, pre-scaled); rows >= R are zero
    for (int e = tid; e < MR * D; e += 256) {
        const int r = e / D, d = e % D;
        qs[r][d] = r < R ? bf2f(reinterpret_cast<const u16*>(q)[((((long)b * T + r / G) * H) + hk * G + r % G) * D + d]) *
                               scale
                         : 0.f;
    }
    __syncthreads();
    // 1. scores: (sum_d q_d k_d) [* k_scale], d ascending (key s0 + tid is visible to row r iff it is <= p0 + r / G)
    {
        float s[MR];
#pragma unroll
        for (int r = 0; r < MR; ++r) s[r] = 0.f;
        if (ok) {
#pragma unroll
            for (int d = 0; d < D; d += Fmt::GR) {
                float kx[Fmt::GR];
#pragma unroll
                for (int i = 0; i < Fmt::GR; ++i) kx[i] = Fmt::key(kr, d + i);
#pragma unroll
                for (int r = 0; r < MR; ++r)
#pragma unroll
                    for (int i = 0; i < Fmt::GR; ++i) s[r] += qs[r][d + i] * kx[i];
            }
        }
        const int key = s0 + tid;
#pragma unroll
        for (int r = 0; r < MR; ++r) {
            if constexpr (Fmt::scaled) s[r] *= ksc;
            ps[r][tid] = (ok && key <= p0 + r / G) ? s[r] : -INFINITY;
        }
    }    __syncthreads();
    // 2. per-row max / exp / sum over the chunk (a row with no visible key here: m = -inf, p = 0); with scales ps
    // takes p * v_scale, the sum l the plain p
    float mg[MR], lg[MR];
#pragma unroll
    for (int r = 0; r < MR; ++r) {
        float m = wave_max(ps[r][tid]);
        if (lane == 0) red[0][wv] = m;
        __syncthreads();
        m = fmaxf(fmaxf(red[0][0], red[0][1]), fmaxf(red[0][2], red[0][3]));
        const float p = (tid < n && m != -INFINITY) ? __expf(ps[r][tid] - m) : 0.f;
        if constexpr (Fmt::scaled) ps[r][tid] = p * vsc;
        else ps[r][tid] = p;
        float sm = wave_sum(p);
        if (lane == 0) red[1][wv] = sm;
        __syncthreads();
        mg[r] = m;
        lg[r] = red[1][0] + red[1][1] + red[1][2] + red[1][3];
        __syncthreads();  // red[] reused by the next row
    }
    // 3. o[r][d] = sum_t p[r][t] V[t][d]; thread = (key partition kp, vector dv)
    float acc[MR][8];
#pragma unroll
    for (int r = 0; r < MR; ++r)
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[r][j] = 0.f;
#pragma unroll
    for (int jj = 0; jj < CH / KP; ++jj) {
        const int t = kp + KP * jj;
        if (t >= n) break;
        const VVec vv = vr[jj];
#pragma unroll
        for (int r = 0; r < MR; ++r) {
            const float p = ps[r][t];
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[r][j] += p * Fmt::val(vv, j);
        }
    }
    // lanes that share dv differ by multiples of DV: butterfly over the wave's key partitions
#pragma unroll
    for (int off = DV; off < 64; off <<= 1)
#pragma unroll
        for (int r = 0; r < MR; ++r)
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[r][j] += __shfl_xor(acc[r][j], off);
    if (lane < DV) {
#pragma unroll
        for (int r = 0; r < MR; ++r)
#pragma unroll
            for (int j = 0; j < 8; ++j) ob[wv][r][dv * 8 + j] = acc[r][j];
    }
    __syncthreads();
    // 4. partial results per row: {o[D], m, l}
    for (int e = tid; e < R * D; e += 256) {
        const int r = e / D, dd = e % D;
        prow(r)[dd] = ob[0][r][dd] + ob[1][r][dd] + ob[2][r][dd] + ob[3][r][dd];
    }
    if (tid < R) {  // the row statistics (registers, identical in every thread)
        float m = mg[0], l = lg[0];
#pragma unroll
        for (int r = 1; r < MR; ++r)
            if (tid == r) { m = mg[r]; l = lg[r]; }
        float* pr = prow(tid);
        pr[D] = m;
        pr[D + 1] = l;
    }
}

template <int D>
__global__ void __launch_bounds__(D) decode_combine_kernel(const float* __restrict__ part, __bf16* __restrict__ out,
                                                           int nsplit) {
    const long bh = blockIdx.x;
    const int d = threadIdx.x;
    const float* p = part + bh * nsplit * (D + 2);
    float M = -INFINITY;
    for (int s = 0; s < nsplit; ++s) M = fmaxf(M, p[s * (D + 2) + D]);
    float Lsum = 0.f, o = 0.f;
    for (int s = 0; s < nsplit; ++s) {
        const float m = p[s * (D + 2) + D];
        if (m == -INFINITY) continue;
        const float c = __expf(m - M);
        Lsum += c * p[s * (D + 2) + D + 1];
        o += c * p[s * (D + 2) + d];
    }
    reinterpret_cast<u16*>(out)[bh * D + d] = f2bf(Lsum > 0.f ? o / Lsum : 0.f);
}

// KV-cache append into the bf16 cache: append_vec's (kv_cache.h) vector goes to q [B*T, H*D] or, roped K / plain V,
// into the caches [B, Hkv, Lmax, D] (paged: the pools, through the block table).
// Map (kv_cache.h): UniformMap, B * T rows of T tokens per sequence, or PackedMap, the rows of several prompts end to
// end, each to its own slot (kv_append_packed); the uniform instantiations take an empty `map`.
template <class Lay, class Map>
__global__ void __launch_bounds__(256) kv_append_kernel(const __bf16* __restrict__ qkv, long ld,
                                                        __bf16* __restrict__ qo, __bf16* __restrict__ Kc,
                                                        __bf16* __restrict__ Vc, const float* __restrict__ cosT,
                                                        const float* __restrict__ sinT, const int* __restrict__ pos,
                                                        int pstride, int T, int H, int Hkv, int D, int Lmax,
                                                        long total, Lay lay, Map map) {
    const int pshared = pos[0];
    for (long idx = blockIdx.x * 256L + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
        AppendVec a;
        if (!append_vec(a, idx, total, qkv, ld, cosT, sinT, pos, pstride, pshared, T, H, Hkv, D, Lmax, lay, map))
            continue;
        __bf16* dst;
        if (a.hh < H) dst = qo + a.r * (long)H * D + (long)a.hh * D + a.d0;
        else dst = (a.hh < H + Hkv ? Kc : Vc) + a.row * D + a.d0;
        *reinterpret_cast<u16x8*>(dst) = a.x;
    }
}

}  // namespace dec
}  // namespace bpe

using namespace bpe::dec;

int kv_page_rows() { return KV_PAGE; }

int decode_attn_splits(int Lmax) { return (Lmax + CH - 1) / CH; }

// T new tokens per sequence: the G * T query rows of a kv head share one workgroup (at most 8)
bool decode_attn_ok(int H, int Hkv, int D, int T) {
    const int G = Hkv > 0 ? H / Hkv : 0;
    return (D == 64 || D == 128) && Hkv > 0 && H % Hkv == 0 && T >= 1 && G >= 1 && G * T <= 8;
}

template <int D, class Fmt, class Lay>
static void launch_d(const void* q, const void* k, const void* v, const float* ks, const float* vs, float* part,
                     void* out, const int* pos, int pstride, int B, int T, int H, int Hkv, int Lmax, float scale,
                     Lay lay, hipStream_t s) {
    const int ns = decode_attn_splits(Lmax);
    const int grid = B * Hkv * ns;
    const int R = (H / Hkv) * T;
#define DEC(MR)                                                                                                   \
    decode_attn_kernel<D, MR, Fmt, Lay><<<grid, 256, 0, s>>>((const __bf16*)q, k, v, ks, vs, part, pos, pstride, H, \
                                                             Hkv, Lmax, ns, scale, T, lay)
    if (R <= 1) DEC(1);
    else if (R <= 2) DEC(2);
    else if (R <= 4) DEC(4);
    else DEC(8);
#undef DEC
    if (out != nullptr) decode_combine_kernel<D><<<B * T * H, D, 0, s>>>(part, (__bf16*)out, ns);
}

template <class Lay>
static void launch_lay(const void* q, const void* k, const void* v, const float* ks, const float* vs, float* part,
                       void* out, const int* pos, int pos_stride, int B, int T, int H, int Hkv, int D, int Lmax,
                       float scale, Lay lay, hipStream_t s) {
    const auto launch = ks != nullptr ? (D == 64 ? launch_d<64, Fp8Cache, Lay> : launch_d<128, Fp8Cache, Lay>)
                                      : (D == 64 ? launch_d<64, Bf16Cache, Lay> : launch_d<128, Bf16Cache, Lay>);
    launch(q, k, v, ks, vs, part, out, pos, pos_stride, B, T, H, Hkv, Lmax, scale, lay, s);
}

void launch_decode_attn(const void* q, const void* k, const void* v, const float* ks, const float* vs, float* part,
                        void* out, const int* pos, int pos_stride, int B, int T, int H, int Hkv, int D, int Lmax,
                        float scale, hipStream_t s, const KvPages& pg) {
    if (pg.table != nullptr)
        launch_lay(q, k, v, ks, vs, part, out, pos, pos_stride, B, T, H, Hkv, D, Lmax, scale,
                   PagedLayout{pg.table, pg.NB, pg.P}, s);
    else launch_lay(q, k, v, ks, vs, part, out, pos, pos_stride, B, T, H, Hkv, D, Lmax, scale, SlabLayout{}, s);
}

// `rows` token rows in all: B * T of the uniform map, N of the packed one
template <class Map>
static void append_launch(const void* qkv, long ld, void* qo, void* Kc, void* Vc, const float* cosT, const float* sinT,
                          const int* pos, int pos_stride, long rows, int T, int H, int Hkv, int D, int Lmax, Map map,
                          hipStream_t s, const KvPages& pg) {
    const long total = rows * (H + 2 * Hkv) * (D / 8);
    const long want = (total + 255) / 256;
    const int grid = (int)(want < 8192 ? want : 8192);
    if (pg.table != nullptr)
        kv_append_kernel<<<grid, 256, 0, s>>>((const __bf16*)qkv, ld, (__bf16*)qo, (__bf16*)Kc, (__bf16*)Vc, cosT,
                                              sinT, pos, pos_stride, T, H, Hkv, D, Lmax, total,
                                              PagedLayout{pg.table, pg.NB, pg.P}, map);
    else
        kv_append_kernel<<<grid, 256, 0, s>>>((const __bf16*)qkv, ld, (__bf16*)qo, (__bf16*)Kc, (__bf16*)Vc, cosT,
                                              sinT, pos, pos_stride, T, H, Hkv, D, Lmax, total, SlabLayout{}, map);
}

void launch_kv_append(const void* qkv, long ld, void* qo, void* Kc, void* Vc, const float* cosT, const float* sinT,
                      const int* pos, int pos_stride, int B, int T, int H, int Hkv, int D, int Lmax, hipStream_t s,
                      const KvPages& pg) {
    append_launch(qkv, ld, qo, Kc, Vc, cosT, sinT, pos, pos_stride, (long)B * T, T, H, Hkv, D, Lmax, UniformMap{}, s,
                  pg);
}

void launch_kv_append_packed(const void* qkv, long ld, void* qo, void* Kc, void* Vc, const float* cosT,
                             const float* sinT, const int* pos, const KvPacked& pk, int B, int H, int Hkv, int D,
                             int Lmax, hipStream_t s, const KvPages& pg) {
    append_launch(qkv, ld, qo, Kc, Vc, cosT, sinT, pos, 1, (long)pk.N, 1, H, Hkv, D, Lmax, PackedMap{pk.seq, pk.S, B},
                  s, pg);
}
