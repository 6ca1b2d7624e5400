// fp8 KV cache of the serving path, gfx950: e4m3 rows with one power-of-two scale each.
//
// A cache row is the D values of one (sequence, kv head, position).  Storage: bytes k8 / v8 [B, Hkv, Lmax, D] (OCP
// e4m3fn, gfx950's encoding) and fp32 scales ks / vs [B, Hkv, Lmax].  The quantiser's input is the row as the bf16
// cache would have held it (K roped and rounded to bf16, V as is).  With a = max_j |x_j|, the scale s is the smallest
// power of two with a / s <= 448: a = 1.M * 2^(E - 127) (fp32 fields) gives s = 2^(E - 135) when M <= 0.75 (a <= 1.75
// * 2^(E - 127) = 448 * 2^(E - 135)), else 2^(E - 134) -- integer work on the exponent and mantissa bits, no
// division, no log2.  s is clamped below at 2^-64, an all-zero row gets s = 1, a row with a non-finite element
// s = NaN (its bytes are unspecified; every consumer then yields NaN, as the bf16 cache would).
//   q_j = e4m3_rne(x_j * (1 / s))   exact product (1 / s is a power of two), never saturates (|x_j / s| <= 448)
//   deq = q_j * s                   exact in fp32 and representable in bf16 (4 significant bits)
// So "the fp8 cache" is "a bf16 cache that holds the dequantised values", and a key's scale can be folded into its
// score, a value's scale into its probability, without changing any rounding (barring underflow).
//
//   kv_append_fp8   kv_append_kernel (decode_attn.hip) with the K / V rows quantised: one thread per 8-element
//                   vector, the D / 8 adjacent lanes of a row reduce the row's amax bits with lane shuffles (groups
//                   are wave-aligned: 64 and 256 are multiples of D / 8), each lane stores its 8 bytes with one
//                   vector store, lane 0 of the group stores the scale.  The roped q is that of kv_append, bit for bit.
//   decode_attn_fp8 decode_attn_kernel with half the bytes per key: a thread loads its key's D bytes in D / 16
//                   16-byte loads plus one fp32 scale, and 8 bytes per (key, 8-wide d) of V; every load is issued at
//                   kernel entry.  k_scale[t] multiplies the score, v_scale[t] the probability p[r][t] (the row sum l
//                   takes the unscaled p).  Partials layout, chunking, empty-chunk rule and combine are the bf16
//                   kernel's (decode_combine_kernel and decode_attn_proj consume the partials unchanged).
//   kv_dequant      rows [0, min(pos[b] + T, Lmax)) of each K and V slab -> bf16 scratch [B, Hkv, Lmax, D] (one
//                   launch for both), rows past that untouched; pos is read on the device.  Feeds cache_attn for the
//                   windows decode_attn_fp8 does not take (G * T >= 9).
//
// Resources (hipcc -O3, gfx950, -Rpass-analysis=kernel-resource-usage), scratch 0 in every kernel; the bf16
// decode_attn_kernel next to it in brackets:
//   decode_attn_fp8_kernel<64, MR>   MR 1 / 2 / 4 / 8:  VGPRs 62 / 80 / 96 / 180    (90 / 107 / 122 / 180)
//   decode_attn_fp8_kernel<128, MR>  MR 1 / 2 / 4 / 8:  VGPRs 94 / 112 / 120 / 180  (154 / 168 / 200 / 242)
//   kv_append_fp8_kernel  VGPRs 44     kv_dequant_kernel  VGPRs 29
#include "common.h"
#include "kernels.h"

typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

namespace bpe {
namespace kv8 {

constexpr int CH = 256;  // keys per chunk (= threads per workgroup), as decode_attn.hip

// two e4m3 bytes of `w` (the low or the high half) -> fp32 (v_cvt_pk_f32_fp8, exact)
__device__ __forceinline__ f32x2 fp8x2(unsigned w, bool hi) {
    return hi ? __builtin_amdgcn_cvt_pk_f32_fp8((int)w, true) : __builtin_amdgcn_cvt_pk_f32_fp8((int)w, false);
}

// The decode_attn_kernel of decode_attn.hip (its comments hold here) reading the fp8 cache.  MR is a template
// parameter for the same reason: per-row registers must be statically indexed.
template <int D, int MR>
__global__ void __launch_bounds__(256)
decode_attn_fp8_kernel(const __bf16* __restrict__ q, const unsigned char* __restrict__ K8,
                       const unsigned char* __restrict__ V8, const float* __restrict__ Ks,
                       const float* __restrict__ Vs, float* __restrict__ part, const int* __restrict__ pos, int pstride,
                       int H, int Hkv, int Lmax, int nsplit, float scale, int T) {
    constexpr int DV = D / 8;     // 8-byte vectors per V row
    constexpr int DK = D / 16;    // 16-byte vectors per K row
    constexpr int KP = 256 / DV;  // key partitions of the P.V step
    __shared__ float qs[MR][D];
    __shared__ float ps[MR][CH];
    __shared__ float red[2][4];
    __shared__ float ob[4][MR][D];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int bk = blockIdx.x / nsplit, split = blockIdx.x % nsplit;  // bk = b * Hkv + hk
    const int b = bk / Hkv, hk = bk % Hkv;
    const int G = H / Hkv, R = G * T;
    const int p0 = pos[b * pstride];
    const int L = min(p0 + T, Lmax);
    const int s0 = split * CH;
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
    const long rowbase = (long)bk * Lmax + s0;  // first cache row of the chunk: bytes at rowbase * D, scales at rowbase
    // every load of the chunk is issued up front: the key's D bytes and scale, the value scale of key tid (folded
    // into p below), and the V bytes of this thread's (key partition, d vector) slots
    const bool ok = tid < n;
    u32x4 kr[DK];
    {
        const u32x4* kp = reinterpret_cast<const u32x4*>(K8 + (rowbase + tid) * D);
#pragma unroll
        for (int v = 0; v < DK; ++v) kr[v] = ok ? kp[v] : u32x4{};
    }
    const float ksc = ok ? Ks[rowbase + tid] : 0.f;
    const float vsc = ok ? Vs[rowbase + tid] : 0.f;
    const int dv = tid % DV, kp = tid / DV;
    u32x2 vr[CH / KP];
#pragma unroll
    for (int j = 0; j < CH / KP; ++j) {
        const int t = kp + KP * j;
        vr[j] = t < n ? *reinterpret_cast<const u32x2*>(V8 + (rowbase + t) * D + dv * 8) : u32x2{};
    }
    // query rows -> LDS (fp32, pre-scaled); rows >= R are zero
    for (int e = tid; e < MR * D; e += 256) {
        const int r = e / D, d = e % D;
        qs[r][d] = r < R ? bf2f(reinterpret_cast<const u16*>(q)[((((long)b * T + r / G) * H) + hk * G + r % G) * D + d]) *
                               scale
                         : 0.f;
    }
    __syncthreads();
    // 1. scores: (sum_d q_d k8_d) * k_scale (key s0 + tid is visible to row r iff it is <= p0 + r / G)
    {
        float s[MR];
#pragma unroll
        for (int r = 0; r < MR; ++r) s[r] = 0.f;
        if (ok) {
#pragma unroll
            for (int v = 0; v < DK; ++v) {
#pragma unroll
                for (int w = 0; w < 4; ++w) {
                    const unsigned word = kr[v][w];
                    const f32x2 lo = fp8x2(word, false), hi = fp8x2(word, true);
                    const int d0 = 16 * v + 4 * w;
#pragma unroll
                    for (int r = 0; r < MR; ++r) {
                        s[r] += qs[r][d0] * lo.x;
                        s[r] += qs[r][d0 + 1] * lo.y;
                        s[r] += qs[r][d0 + 2] * hi.x;
                        s[r] += qs[r][d0 + 3] * hi.y;
                    }
                }
            }
        }
        const int key = s0 + tid;
#pragma unroll
        for (int r = 0; r < MR; ++r) ps[r][tid] = (ok && key <= p0 + r / G) ? s[r] * ksc : -INFINITY;
    }
    __syncthreads();
    // 2. per-row max / exp / sum over the chunk; ps takes p * v_scale, the sum l the plain p
    float mg[MR], lg[MR];
#pragma unroll
    for (int r = 0; r < MR; ++r) {
        float m = wave_max(ps[r][tid]);
        if (lane == 0) red[0][wv] = m;
        __syncthreads();
        m = fmaxf(fmaxf(red[0][0], red[0][1]), fmaxf(red[0][2], red[0][3]));
        const float p = (tid < n && m != -INFINITY) ? __expf(ps[r][tid] - m) : 0.f;
        ps[r][tid] = p * vsc;
        float sm = wave_sum(p);
        if (lane == 0) red[1][wv] = sm;
        __syncthreads();
        mg[r] = m;
        lg[r] = red[1][0] + red[1][1] + red[1][2] + red[1][3];
        __syncthreads();  // red[] reused by the next row
    }
    // 3. o[r][d] = sum_t (p[r][t] v_scale[t]) v8[t][d]; thread = (key partition kp, vector dv)
    float acc[MR][8];
#pragma unroll
    for (int r = 0; r < MR; ++r)
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[r][j] = 0.f;
#pragma unroll
    for (int jj = 0; jj < CH / KP; ++jj) {
        const int t = kp + KP * jj;
        if (t >= n) break;
        const u32x2 vv = vr[jj];
        const f32x2 v0 = fp8x2(vv.x, false), v1 = fp8x2(vv.x, true), v2 = fp8x2(vv.y, false), v3 = fp8x2(vv.y, true);
        const float vf[8] = {v0.x, v0.y, v1.x, v1.y, v2.x, v2.y, v3.x, v3.y};
#pragma unroll
        for (int r = 0; r < MR; ++r) {
            const float p = ps[r][t];
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[r][j] += p * vf[j];
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

// Scale of a row from the largest |x| bits of its bf16 elements (integer order = magnitude order, and inf / NaN
// sort above every finite value): -> s, and 1 / s in `inv`.
__device__ __forceinline__ float row_scale(unsigned amax16, float& inv) {
    if (amax16 >= 0x7f80u) {  // a non-finite element
        inv = 0.f;
        return __uint_as_float(0x7fc00000u);
    }
    if (amax16 == 0u) {
        inv = 1.f;
        return 1.f;
    }
    const int E = (int)(amax16 >> 7), M = (int)(amax16 & 0x7f);  // fp32 exponent field, top 7 mantissa bits
    const int sf = max(E - 8 + (M > 0x60 ? 1 : 0), 63);          // exponent field of s, clamped at 2^-64
    inv = __uint_as_float((unsigned)(254 - sf) << 23);
    return __uint_as_float((unsigned)sf << 23);
}

// kv_append_kernel with quantised K / V rows.  The loop bound is uniform per workgroup and every lane runs the
// shuffles, so the D / 8 lanes of a row (same r, same head: all active or all skipped together) always find each
// other; a lane with nothing to do carries zeros.
__global__ void __launch_bounds__(256)
kv_append_fp8_kernel(const __bf16* __restrict__ qkv, long ld, __bf16* __restrict__ qo, unsigned char* __restrict__ K8,
                     unsigned char* __restrict__ V8, float* __restrict__ Ks, float* __restrict__ Vs,
                     const float* __restrict__ cosT, const float* __restrict__ sinT, const int* __restrict__ pos,
                     int pstride, int T, int H, int Hkv, int D, int Lmax, long total) {
    const int dv = D / 8, W = (H + 2 * Hkv) * dv;
    const int pshared = pos[0];
    for (long base = blockIdx.x * 256L; base < total; base += (long)gridDim.x * 256) {
        const long idx = base + threadIdx.x;
        const bool in = idx < total;
        const long r = in ? idx / W : 0;
        const int c = in ? (int)(idx % W) : 0, hh = c / dv, d0 = (c % dv) * 8;
        const int b = (int)(r / T);
        const int p = (pstride ? pos[b] : pshared) + (int)(r % T);
        const bool act = in && p < Lmax;  // cache full: nothing is written past the end
        u16x8 x = {};
        if (act) {
            x = *reinterpret_cast<const u16x8*>(qkv + r * ld + (long)hh * D + d0);
            if (hh < H + Hkv && cosT != nullptr) {
                const float* cs = cosT + (long)p * (D / 2) + d0 / 2;
                const float* sn = sinT + (long)p * (D / 2) + d0 / 2;
#pragma unroll
                for (int j = 0; j < 8; j += 2) {
                    const float x1 = bf2f(x[j]), x2 = bf2f(x[j + 1]), cc = cs[j / 2], ss = sn[j / 2];
                    x[j] = f2bf(x1 * cc - x2 * ss);
                    x[j + 1] = f2bf(x1 * ss + x2 * cc);
                }
            }
        }
        unsigned am = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j) am = max(am, (unsigned)(x[j] & 0x7fff));
        for (int off = 1; off < dv; off <<= 1) am = max(am, (unsigned)__shfl_xor((int)am, off));
        if (!act) continue;
        if (hh < H) {
            *reinterpret_cast<u16x8*>(qo + r * (long)H * D + (long)hh * D + d0) = x;
            continue;
        }
        float inv;
        const float s = row_scale(am, inv);
        u32x2 w;
        w.x = (unsigned)__builtin_amdgcn_cvt_pk_fp8_f32(bf2f(x[0]) * inv, bf2f(x[1]) * inv, 0, false);
        w.x = (unsigned)__builtin_amdgcn_cvt_pk_fp8_f32(bf2f(x[2]) * inv, bf2f(x[3]) * inv, (int)w.x, true);
        w.y = (unsigned)__builtin_amdgcn_cvt_pk_fp8_f32(bf2f(x[4]) * inv, bf2f(x[5]) * inv, 0, false);
        w.y = (unsigned)__builtin_amdgcn_cvt_pk_fp8_f32(bf2f(x[6]) * inv, bf2f(x[7]) * inv, (int)w.y, true);
        const bool isk = hh < H + Hkv;
        const long row = ((long)b * Hkv + (isk ? hh - H : hh - H - Hkv)) * Lmax + p;
        *reinterpret_cast<u32x2*>((isk ? K8 : V8) + row * D + d0) = w;
        if (d0 == 0) (isk ? Ks : Vs)[row] = s;
    }
}

// One thread per 16 bytes of a K or V row: rows below min(pos[b] + T, Lmax) -> bf16, the others skipped.
__global__ void __launch_bounds__(256)
kv_dequant_kernel(const unsigned char* __restrict__ K8, const unsigned char* __restrict__ V8,
                  const float* __restrict__ Ks, const float* __restrict__ Vs, __bf16* __restrict__ Ko,
                  __bf16* __restrict__ Vo, const int* __restrict__ pos, int pstride, int T, int Hkv, int D, int Lmax,
                  long rows) {
    const int dk = D / 16;
    const long total = 2 * rows * dk;  // K rows, then V rows
    const int pshared = pos[0];
    for (long idx = blockIdx.x * 256L + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
        const long rr = idx / dk;
        const int d0 = (int)(idx % dk) * 16;
        const bool isv = rr >= rows;
        const long row = isv ? rr - rows : rr;  // (b * Hkv + hk) * Lmax + t
        const int t = (int)(row % Lmax), b = (int)(row / ((long)Lmax * Hkv));
        const int p = pstride ? pos[b] : pshared;
        if (t >= min(p + T, Lmax)) continue;
        const u32x4 w = *reinterpret_cast<const u32x4*>((isv ? V8 : K8) + row * D + d0);
        const float s = (isv ? Vs : Ks)[row];
        u16x8 lo, hi;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const f32x2 a = fp8x2(w[i], false), c = fp8x2(w[i], true);
            lo[4 * i] = f2bf(a.x * s); lo[4 * i + 1] = f2bf(a.y * s);
            lo[4 * i + 2] = f2bf(c.x * s); lo[4 * i + 3] = f2bf(c.y * s);
            const f32x2 e = fp8x2(w[2 + i], false), g = fp8x2(w[2 + i], true);
            hi[4 * i] = f2bf(e.x * s); hi[4 * i + 1] = f2bf(e.y * s);
            hi[4 * i + 2] = f2bf(g.x * s); hi[4 * i + 3] = f2bf(g.y * s);
        }
        u16x8* dst = reinterpret_cast<u16x8*>((isv ? Vo : Ko) + row * D + d0);
        dst[0] = lo;
        dst[1] = hi;
    }
}

}  // namespace kv8
}  // namespace bpe

using namespace bpe::kv8;

template <int D>
static void launch_d(const void* q, const void* k8, const void* v8, const float* ks, const float* vs, float* part,
                     void* out, const int* pos, int pstride, int B, int T, int H, int Hkv, int Lmax, float scale,
                     hipStream_t s) {
    const int ns = decode_attn_splits(Lmax);
    const int grid = B * Hkv * ns;
    const int R = (H / Hkv) * T;
#define DEC(MR)                                                                                                    \
    decode_attn_fp8_kernel<D, MR><<<grid, 256, 0, s>>>((const __bf16*)q, (const unsigned char*)k8,                  \
                                                       (const unsigned char*)v8, ks, vs, part, pos, pstride, H, Hkv, \
                                                       Lmax, ns, scale, T)
    if (R <= 1) DEC(1);
    else if (R <= 2) DEC(2);
    else if (R <= 4) DEC(4);
    else DEC(8);
#undef DEC
    if (out != nullptr) launch_decode_combine(part, out, B * T * H, D, ns, s);
}

void launch_decode_attn_fp8(const void* q, const void* k8, const void* v8, const float* ks, const float* vs,
                            float* part, void* out, const int* pos, int pos_stride, int B, int T, int H, int Hkv,
                            int D, int Lmax, float scale, hipStream_t s) {
    if (D == 64) launch_d<64>(q, k8, v8, ks, vs, part, out, pos, pos_stride, B, T, H, Hkv, Lmax, scale, s);
    else launch_d<128>(q, k8, v8, ks, vs, part, out, pos, pos_stride, B, T, H, Hkv, Lmax, scale, s);
}

void launch_kv_append_fp8(const void* qkv, long ld, void* qo, void* k8, void* v8, float* ks, float* vs,
                          const float* cosT, const float* sinT, const int* pos, int pos_stride, int B, int T, int H,
                          int Hkv, int D, int Lmax, hipStream_t s) {
    const long total = (long)B * T * (H + 2 * Hkv) * (D / 8);
    const long want = (total + 255) / 256;
    const int grid = (int)(want < 8192 ? want : 8192);
    kv_append_fp8_kernel<<<grid, 256, 0, s>>>((const __bf16*)qkv, ld, (__bf16*)qo, (unsigned char*)k8,
                                              (unsigned char*)v8, ks, vs, cosT, sinT, pos, pos_stride, T, H, Hkv, D,
                                              Lmax, total);
}

void launch_kv_dequant(const void* k8, const void* v8, const float* ks, const float* vs, void* ko, void* vo,
                       const int* pos, int pos_stride, int B, int T, int Hkv, int D, int Lmax, hipStream_t s) {
    const long rows = (long)B * Hkv * Lmax;
    const long want = (2 * rows * (D / 16) + 255) / 256;
    const int grid = (int)(want < 8192 ? want : 8192);
    kv_dequant_kernel<<<grid, 256, 0, s>>>((const unsigned char*)k8, (const unsigned char*)v8, ks, vs, (__bf16*)ko,
                                           (__bf16*)vo, pos, pos_stride, T, Hkv, D, Lmax, rows);
}
