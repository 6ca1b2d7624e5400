// What the two KV-cache formats of the serving path share, and the little in which they differ (gfx950).
//
//   bf16   K / V [B, Hkv, Lmax, D] bf16 (K roped)
//   fp8    the same rows as D e4m3 bytes plus one power-of-two fp32 scale per row, ks / vs [B, Hkv, Lmax]
//          (kv_fp8.hip states the format)
//
// decode_attn_kernel (decode_attn.hip) is written once against a format policy -- Bf16Cache / Fp8Cache below: the
// register types of a key row and of a V slot, where a row starts, element d of either as fp32, and whether a row
// carries a scale.  The two append kernels (kv_append_kernel in decode_attn.hip, kv_append_fp8_kernel in kv_fp8.hip)
// share append_vec: which 8 values a thread handles, RoPE'd, and where they go.
//
// Beside the format there is the LAYOUT -- where cache row (b, kv head, position) lies -- as a second policy, SlabLayout
// / PagedLayout below.  The slab is the [B, Hkv, Lmax, D] tensor above.  The paged cache is a pool of pages
//   K / V [P, Hkv, KV_PAGE, D] (either format; fp8 scales [P, Hkv, KV_PAGE])
// and an int32 block table [B, NB], NB * KV_PAGE >= Lmax: entry [b, j] is the pool page that holds positions
// KV_PAGE * j .. KV_PAGE * j + KV_PAGE - 1 of sequence b, -1 where none is allocated.  KV_PAGE is decode_attn's chunk
// and four of cache_attn's 64-key tiles, so a chunk is one page and a tile never straddles one: the indirection is
// one table entry per chunk / per four tiles, and the arithmetic on the rows, and its order, is the slab kernels'.
// The table is device data like pos, and no content of either may address outside the pool: a reader clamps the page
// id into [0, P - 1] (page_clamped), a writer whose entry is outside [0, P) writes nothing (paged_row).  The layout
// is a compile-time property: the slab instantiations take an empty argument and are the code they were.
//
// A third policy is the token MAP -- which sequence and which of its tokens a row of q / qkv is.  UniformMap: B
// sequences of T tokens each, row b * T + t, the cache slot is b.  PackedMap: the prompts of several sequences laid
// end to end with no padding, described by a host-written device int32 table [S, 3] of (slot, off, n) -- the cache
// slot (row of pos, of the slab batch and of the block table), the sequence's first packed row and its token count;
// offs ascend and off[i + 1] = off[i] + n[i].  The position of a packed sequence is pos[slot], read on the device.
// Like the layout it is a compile-time property, and the uniform instantiations take an empty argument.
#pragma once
#include "common.h"

typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

namespace bpe {
namespace kvc {

constexpr int KV_PAGE = 256;  // rows of a page (= dec::CH, a multiple of cache_attn's 64-key tile)

struct SlabLayout {
    static constexpr bool paged = false;
};

struct PagedLayout {
    static constexpr bool paged = true;
    const int* table;  // [B, NB]
    int NB, P;         // table columns (NB * KV_PAGE >= Lmax), pages in the pool
    // the page of positions KV_PAGE * j .. of sequence b for a reader, clamped into the pool (0 <= j < NB)
    __device__ __forceinline__ int page_clamped(int b, int j) const {
        return min(max(table[(long)b * NB + j], 0), P - 1);
    }
    // the pool row of position p (0 <= p < NB * KV_PAGE) of (sequence b, kv head hk) for a writer, or -1 where the
    // table has no page in [0, P) for it
    __device__ __forceinline__ long row(int b, int hk, int Hkv, int p) const {
        const int pg = table[(long)b * NB + p / KV_PAGE];
        if ((unsigned)pg >= (unsigned)P) return -1;
        return ((long)pg * Hkv + hk) * KV_PAGE + p % KV_PAGE;
    }
};

struct UniformMap {
    static constexpr bool packed = false;
};

struct PackedMap {
    static constexpr bool packed = true;
    const int* seq;  // [S, 3]: (slot, off, n) per sequence
    int S, B;        // sequences; slots of the cache (slot ids are checked on the host and clamped here)
    __device__ __forceinline__ int slot(int i) const { return min(max(seq[3 * i], 0), B - 1); }
    __device__ __forceinline__ int off(int i) const { return seq[3 * i + 1]; }
    __device__ __forceinline__ int n(int i) const { return seq[3 * i + 2]; }
    // the sequence that holds packed row r (0 <= r < N): the last one whose off is <= r
    __device__ __forceinline__ int find(int r) const {
        int lo = 0, hi = S - 1;
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (off(mid) <= r) lo = mid;
            else hi = mid - 1;
        }
        return lo;
    }
};

// two e4m3 bytes of `w` (the low or the high half) -> fp32 (v_cvt_pk_f32_fp8, exact)
__device__ __forceinline__ f32x2 fp8x2(unsigned w, bool hi) {
    return hi ? __builtin_amdgcn_cvt_pk_f32_fp8((int)w, true) : __builtin_amdgcn_cvt_pk_f32_fp8((int)w, false);
}

// A policy names the stored element (`elem`: a cache row is D of them), the 16-byte register of a key row (`KVec`,
// KE elements) and the register that holds the 8 elements of a V slot (`VVec`); `key` / `val` give element d of a
// key row / j of a V slot as fp32 (constant indices after unrolling; repeated conversions of one register fold).
// `scaled`: a row has a scale, which the kernel loads and applies.
// Two members are there for register allocation only (VGPR counts decide the occupancy here; decode_attn.hip's
// table): `row`, the address of cache row rowbase + t in the association that instantiation allocates best with,
// and `GR`, how many key elements the score loop converts before it runs over the query rows (a bf16 element is one
// shift, an e4m3 word converts to four floats).  With the other format's choice of either, fp8 <64, 2> and <64, 4>
// and bf16 <128, 2> each take a few more VGPRs and lose a wave per SIMD; no result depends on them.
struct Bf16Cache {
    static constexpr bool scaled = false;
    typedef u16 elem;
    typedef u16x8 KVec;
    typedef u16x8 VVec;
    static constexpr int KE = 8, GR = 1;
    static __device__ __forceinline__ const elem* row(const void* c, long rowbase, int t, int D) {
        return static_cast<const elem*>(c) + rowbase * D + (long)t * D;
    }
    static __device__ __forceinline__ float val(VVec v, int j) { return bf2f(v[j]); }
    template <int N> static __device__ __forceinline__ float key(const KVec (&kr)[N], int d) {
        return bf2f(kr[d / 8][d % 8]);
    }
};

struct Fp8Cache {
    static constexpr bool scaled = true;
    typedef unsigned char elem;
    typedef u32x4 KVec;
    typedef u32x2 VVec;
    static constexpr int KE = 16, GR = 4;
    static __device__ __forceinline__ const elem* row(const void* c, long rowbase, int t, int D) {
        return static_cast<const elem*>(c) + (rowbase + t) * D;
    }
    static __device__ __forceinline__ float byte(unsigned w, int i) { return fp8x2(w, i >= 2)[i % 2]; }
    static __device__ __forceinline__ float val(VVec v, int j) { return byte(v[j / 4], j % 4); }
    template <int N> static __device__ __forceinline__ float key(const KVec (&kr)[N], int d) {
        return byte(kr[d / 16][(d % 16) / 4], d % 4);
    }
};

// KV-cache append, the part both formats share.  Fused-QKV rows [B*T, (H + 2*Hkv)*D] (row stride ld) of T new tokens
// per sequence at positions *pos .. *pos+T-1; one thread per 16-byte vector (8 bf16) of a row; the rotation pairs
// (2i, 2i+1) never straddle a vector.  Vector `idx` of `total` is head hh (q heads, then K heads, then V heads) of
// token row r, elements d0 .. d0 + 7, roped where q or K (cosT null: no RoPE), and, where K or V, belongs to cache
// row `row` = (b * Hkv + kv head) * Lmax + position (slab), or the pool row PagedLayout::row gives for it.
struct AppendVec {
    u16x8 x;
    long r, row;
    int hh, d0;
};

// -> false (a.x zero) when the thread has nothing to write: idx past the end, or the token's position at or past Lmax
// (cache full: nothing is written past the end; per sequence, like the position itself).  `pshared` = pos[0].
// Paged: also a negative position (pos is device data), and a K or V vector whose table entry is no page of the pool
// (the D / 8 vectors of a row share the entry, so a row is written or dropped as a whole).
// Packed (PackedMap): row r is token r - off_i of the sequence i that holds it, at position pos[slot_i] + r - off_i of
// slot slot_i; T, pstride and pshared are not read.  A negative position is dropped like one at or past Lmax.
template <class Lay = SlabLayout, class Map = UniformMap>
__device__ __forceinline__ bool append_vec(AppendVec& a, long idx, long total, const __bf16* __restrict__ qkv, long ld,
                                           const float* __restrict__ cosT, const float* __restrict__ sinT,
                                           const int* __restrict__ pos, int pstride, int pshared, int T, int H, int Hkv,
                                           int D, int Lmax, const Lay& lay = Lay{}, const Map& map = Map{}) {
    a.x = u16x8{};
    if (idx >= total) return false;
    const int dv = D / 8, W = (H + 2 * Hkv) * dv;
    a.r = idx / W;
    const int c = (int)(idx % W);
    a.hh = c / dv;
    a.d0 = (c % dv) * 8;
    int b, p;
    if constexpr (Map::packed) {
        const int i = map.find((int)a.r);
        b = map.slot(i);
        p = pos[b] + ((int)a.r - map.off(i));
        if (p < 0) return false;
    } else {
        b = (int)(a.r / T);
        p = (pstride ? pos[b] : pshared) + (int)(a.r % T);
    }
    if (p >= Lmax) return false;
    if constexpr (Lay::paged) {
        if (p < 0) return false;
        a.row = 0;
        if (a.hh >= H) {  // (a q vector has no cache row)
            a.row = lay.row(b, a.hh < H + Hkv ? a.hh - H : a.hh - H - Hkv, Hkv, p);
            if (a.row < 0) return false;
        }
    } else {
        a.row = ((long)b * Hkv + (a.hh < H + Hkv ? a.hh - H : a.hh - H - Hkv)) * Lmax + p;
    }
    a.x = *reinterpret_cast<const u16x8*>(qkv + a.r * ld + (long)a.hh * D + a.d0);
    if (a.hh < H + Hkv && cosT != nullptr) {
        const float* cs = cosT + (long)p * (D / 2) + a.d0 / 2;
        const float* sn = sinT + (long)p * (D / 2) + a.d0 / 2;
#pragma unroll
        for (int j = 0; j < 8; j += 2) {
            const float x1 = bf2f(a.x[j]), x2 = bf2f(a.x[j + 1]), cc = cs[j / 2], ss = sn[j / 2];
            a.x[j] = f2bf(x1 * cc - x2 * ss);
            a.x[j + 1] = f2bf(x1 * ss + x2 * cc);
        }
    }
    return true;
}

}  // namespace kvc
}  // namespace bpe
