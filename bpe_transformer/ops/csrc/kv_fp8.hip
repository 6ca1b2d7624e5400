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
//                   vector (append_vec of kv_cache.h, shared with kv_append_kernel: the roped q is that of kv_append
//                   by construction), the D / 8 adjacent lanes of a row reduce the row's amax bits with lane shuffles
//                   (groups are wave-aligned: 64 and 256 are multiples of D / 8), each lane stores its 8 bytes with
//                   one vector store, lane 0 of the group stores the scale.
//   kv_dequant      rows [0, min(pos[b] + T, Lmax)) of each K and V slab -> a caller's bf16 pair [B, Hkv, Lmax, D]
//                   (one launch for both), rows past that untouched; pos is read on the device.  A utility, and the
//                   oracle of cache_attn's fp8 instantiation, which is bit for bit cache_attn on what this writes.
// The attention over this cache is the Fp8Cache instantiation of decode_attn_kernel (decode_attn.hip, which also
// holds the resource table of all these kernels) for G * T <= 8 query rows per kv head and that of cache_attn_kernel
// (flash_attn_cache.hip: e4m3 tiles converted into the bf16 LDS image) beyond; no session dequantises into memory.
#include "kv_cache.h"
#include "kernels.h"

namespace bpe {
namespace kv8 {

using namespace kvc;

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

// kv_append_kernel (decode_attn.hip) with quantised K / V rows.  The loop bound is uniform per workgroup and every
// lane runs the shuffles, so the D / 8 lanes of a row (same r, same head: all active or all skipped together) always
// find each other; a lane with nothing to do carries zeros.
// Map (kv_cache.h): the uniform rows or the packed ones (kv_append_packed_fp8), as in kv_append_kernel.
template <class Lay, class Map>
__global__ void __launch_bounds__(256)
kv_append_fp8_kernel(const __bf16* __restrict__ qkv, long ld, __bf16* __restrict__ qo, unsigned char* __restrict__ K8,
                     unsigned char* __restrict__ V8, float* __restrict__ Ks, float* __restrict__ Vs,
                     const float* __restrict__ cosT, const float* __restrict__ sinT, const int* __restrict__ pos,
                     int pstride, int T, int H, int Hkv, int D, int Lmax, long total, Lay lay, Map map) {
    const int dv = D / 8;
    const int pshared = pos[0];
    for (long base = blockIdx.x * 256L; base < total; base += (long)gridDim.x * 256) {
        AppendVec a;
        const bool act = append_vec(a, base + threadIdx.x, total, qkv, ld, cosT, sinT, pos, pstride, pshared, T, H,
                                    Hkv, D, Lmax, lay, map);
        const u16x8 x = a.x;
        unsigned am = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j) am = max(am, (unsigned)(x[j] & 0x7fff));
        for (int off = 1; off < dv; off <<= 1) am = max(am, (unsigned)__shfl_xor((int)am, off));
        if (!act) continue;
        if (a.hh < H) {
            *reinterpret_cast<u16x8*>(qo + a.r * (long)H * D + (long)a.hh * D + a.d0) = x;
            continue;
        }
        float inv;
        const float s = row_scale(am, inv);
        u32x2 w;
        w.x = (unsigned)__builtin_amdgcn_cvt_pk_fp8_f32(bf2f(x[0]) * inv, bf2f(x[1]) * inv, 0, false);
        w.x = (unsigned)__builtin_amdgcn_cvt_pk_fp8_f32(bf2f(x[2]) * inv, bf2f(x[3]) * inv, (int)w.x, true);
        w.y = (unsigned)__builtin_amdgcn_cvt_pk_fp8_f32(bf2f(x[4]) * inv, bf2f(x[5]) * inv, 0, false);
        w.y = (unsigned)__builtin_amdgcn_cvt_pk_fp8_f32(bf2f(x[6]) * inv, bf2f(x[7]) * inv, (int)w.y, true);
        const bool isk = a.hh < H + Hkv;
        *reinterpret_cast<u32x2*>((isk ? K8 : V8) + a.row * D + a.d0) = w;
        if (a.d0 == 0) (isk ? Ks : Vs)[a.row] = s;
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

// `rows` token rows in all: B * T of the uniform map, N of the packed one
template <class Map>
static void append8_launch(const void* qkv, long ld, void* qo, void* k8, void* v8, float* ks, float* vs,
                           const float* cosT, const float* sinT, const int* pos, int pos_stride, long rows, int T,
                           int H, int Hkv, int D, int Lmax, Map map, hipStream_t s, const KvPages& pg) {
    const long total = rows * (H + 2 * Hkv) * (D / 8);
    const long want = (total + 255) / 256;
    const int grid = (int)(want < 8192 ? want : 8192);
    if (pg.table != nullptr)
        kv_append_fp8_kernel<<<grid, 256, 0, s>>>((const __bf16*)qkv, ld, (__bf16*)qo, (unsigned char*)k8,
                                                  (unsigned char*)v8, ks, vs, cosT, sinT, pos, pos_stride, T, H, Hkv,
                                                  D, Lmax, total, PagedLayout{pg.table, pg.NB, pg.P}, map);
    else
        kv_append_fp8_kernel<<<grid, 256, 0, s>>>((const __bf16*)qkv, ld, (__bf16*)qo, (unsigned char*)k8,
                                                  (unsigned char*)v8, ks, vs, cosT, sinT, pos, pos_stride, T, H, Hkv,
                                                  D, Lmax, total, SlabLayout{}, map);
}

void launch_kv_append_fp8(const void* qkv, long ld, void* qo, void* k8, void* v8, float* ks, float* vs,
                          const float* cosT, const float* sinT, const int* pos, int pos_stride, int B, int T, int H,
                          int Hkv, int D, int Lmax, hipStream_t s, const KvPages& pg) {
    append8_launch(qkv, ld, qo, k8, v8, ks, vs, cosT, sinT, pos, pos_stride, (long)B * T, T, H, Hkv, D, Lmax,
                   UniformMap{}, s, pg);
}

void launch_kv_append_packed_fp8(const void* qkv, long ld, void* qo, void* k8, void* v8, float* ks, float* vs,
                                 const float* cosT, const float* sinT, const int* pos, const KvPacked& pk, int B, int H,
                                 int Hkv, int D, int Lmax, hipStream_t s, const KvPages& pg) {
    append8_launch(qkv, ld, qo, k8, v8, ks, vs, cosT, sinT, pos, 1, (long)pk.N, 1, H, Hkv, D, Lmax,
                   PackedMap{pk.seq, pk.S, B}, s, pg);
}

void launch_kv_dequant(const void* k8, const void* v8, const float* ks, const float* vs, void* ko, void* vo,
                       const int* pos, int pos_stride, int B, int T, int Hkv, int D, int Lmax, hipStream_t s) {
    const long rows = (long)B * Hkv * Lmax;
    const long want = (2 * rows * (D / 16) + 255) / 256;
    const int grid = (int)(want < 8192 ? want : 8192);
    kv_dequant_kernel<<<grid, 256, 0, s>>>((const unsigned char*)k8, (const unsigned char*)v8, ks, vs, (__bf16*)ko,
                                           (__bf16*)vo, pos, pos_stride, T, Hkv, D, Lmax, rows);
}
