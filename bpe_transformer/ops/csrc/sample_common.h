// Device helpers shared by sample.hip, sample_rows.hip and spec_verify.hip: one 1024-thread workgroup per logits row.
//
//   * RowT / Ctx: a row of bf16 or fp32 logits that starts at any element offset, addressed in "virtual" 16-byte
//     vectors that ARE aligned (sample.hip's header comment has the scheme); nothing outside [0, V) is touched.
//   * Philox4x32-10 and the uniform it gives.
//   * row_argmax: highest order-preserving key, lowest index among equals.
//   * row_total / prefix_find: masses as 64-bit fixed point (z * 2^40, z <= 1).  Integer sums do not depend on the
//     order of the adds, so totals and the index-order inverse-CDF pick give the same bits every run.
//   * Filt / radix_select / cut_ties: the top-k and top-p cut; sample_row: one row's token, min-p included.
//
// Everything lives in an unnamed namespace: each including file gets its own copy.
#pragma once
#include "common.h"
#include "kernels.h"

namespace bpe {
namespace {

typedef unsigned long long u64;

constexpr int S_NT = 1024, S_NW = S_NT / 64, S_REP = 32, S_BINS = 256;
constexpr float S_FIX = 1099511627776.f;  // 2^40

// dynamic LDS layout (bytes)
constexpr int L_CNT = 0;                                 // unsigned [256][32]
constexpr int L_MASS = L_CNT + S_BINS * S_REP * 4;       // u64 [256][32]; the tile sums of a prefix search alias it
constexpr int L_SEL = L_MASS + S_BINS * S_REP * 8;       // u64 [256] bins summed over replicas (count or mass)
constexpr int L_CNTR = L_SEL + S_BINS * 8;               // unsigned [256]
constexpr int L_SCAL = L_CNTR + S_BINS * 4;              // u64 [8] broadcast scalars
constexpr int L_WRED = L_SCAL + 64;                      // unsigned [2][16] argmax partials
constexpr int L_TOTAL = L_WRED + 2 * S_NW * 4;
static_assert(SAMPLE_MAX_TILES * 8 <= S_BINS * S_REP * 8, "tile sums alias the mass histogram");

template <typename T> struct RowT;
template <> struct RowT<__bf16> {
    static constexpr int VEC = 8, KB = 16;
    typedef u16 raw_t;
    static __device__ __forceinline__ unsigned key(unsigned h) {
        if (h == 0x8000u) h = 0;  // -0 ranks with +0
        return (h & 0x8000u) ? (~h & 0xFFFFu) : (h | 0x8000u);
    }
    static __device__ __forceinline__ float val(unsigned h) { return bf2f((u16)h); }
    static __device__ __forceinline__ float key_val(unsigned k) {
        return bf2f((u16)((k & 0x8000u) ? (k ^ 0x8000u) : (~k & 0xFFFFu)));
    }
};
template <> struct RowT<float> {
    static constexpr int VEC = 4, KB = 32;
    typedef unsigned raw_t;
    static __device__ __forceinline__ unsigned key(unsigned b) {
        if (b == 0x80000000u) b = 0;
        return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
    }
    static __device__ __forceinline__ float val(unsigned b) { return __uint_as_float(b); }
    static __device__ __forceinline__ float key_val(unsigned k) {
        return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);
    }
};

__device__ __forceinline__ u64 wave_sum64(u64 v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ u64 wave_scan64(u64 v, int lane) {  // inclusive
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const u64 t = __shfl_up(v, o, 64);
        if (lane >= o) v += t;
    }
    return v;
}

// Philox4x32-10, first output word
__device__ __forceinline__ unsigned philox_x0(unsigned k0, unsigned k1, unsigned c0, unsigned c1, unsigned c2,
                                              unsigned c3) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const u64 p0 = (u64)0xD2511F53u * c0, p1 = (u64)0xCD9E8D57u * c2;
        const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n1 = (unsigned)p1;
        const unsigned n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1, n3 = (unsigned)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return c0;
}

// the uniform of key `seed` at counter (count, row, stream): ((x0 >> 8) + 0.5) * 2^-24
__device__ __forceinline__ float philox_u(u64 seed, u64 count, unsigned row, unsigned stream) {
    const unsigned x0 = philox_x0((unsigned)seed, (unsigned)(seed >> 32), (unsigned)count, (unsigned)(count >> 32),
                                  row, stream);
    return ((float)(x0 >> 8) + 0.5f) * 5.9604644775390625e-8f;  // 2^-24 (one rounding, of the sum)
}

template <typename T> struct Ctx {
    typedef RowT<T> R;
    const typename R::raw_t* p0;  // 16-byte aligned: row start minus off elements
    int off, V, nvec, ntiles;
    float xmax, invT;
    char* smem;
    int lane, wave;

    // row `row` of a dense [rows][V] array that may itself start at any element
    __device__ __forceinline__ void init(const void* base, long row, int V_, char* smem_) {
        const typename R::raw_t* xr = reinterpret_cast<const typename R::raw_t*>(base) + row * V_;
        off = (int)((reinterpret_cast<uintptr_t>(xr) / sizeof(typename R::raw_t)) % R::VEC);
        p0 = xr - off;
        V = V_;
        nvec = (off + V_ + R::VEC - 1) / R::VEC;
        ntiles = (nvec + 63) / 64;
        smem = smem_;
        lane = threadIdx.x & 63;
        wave = threadIdx.x >> 6;
    }
    // raw bits of element i, 0 <= i < V
    __device__ __forceinline__ unsigned at(int i) const { return p0[off + i]; }

    // virtual vector v: raw bits of its elements and which of them are inside the row
    __device__ __forceinline__ unsigned load(int v, unsigned (&raw)[R::VEC]) const {
        const int j0 = v * R::VEC;
        if (j0 >= off && j0 + R::VEC <= off + V) {
            if constexpr (R::VEC == 8) {
                const u16x8 t = *reinterpret_cast<const u16x8*>(p0 + j0);
#pragma unroll
                for (int e = 0; e < 8; ++e) raw[e] = t[e];
            } else {
                typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
                const u32x4 t = *reinterpret_cast<const u32x4*>(p0 + j0);
#pragma unroll
                for (int e = 0; e < 4; ++e) raw[e] = t[e];
            }
            return (1u << R::VEC) - 1;
        }
        unsigned m = 0;  // the unaligned head / the tail of the row: element by element, inside [0, V) only
#pragma unroll
        for (int e = 0; e < R::VEC; ++e) {
            const int i = j0 + e - off;
            raw[e] = 0;
            if (i >= 0 && i < V) { raw[e] = p0[j0 + e]; m |= 1u << e; }
        }
        return m;
    }
    __device__ __forceinline__ u64 zq(unsigned raw) const {  // fixed-point weight of one logit
        const float z = fminf(__expf((R::val(raw) - xmax) * invT), 1.f);
        return (u64)(z * S_FIX);
    }
    __device__ __forceinline__ u64* scal() const { return reinterpret_cast<u64*>(smem + L_SCAL); }
};

// argmax of the row: the highest key and the lowest index that has it, in every thread.  One barrier; the partials
// (L_WRED) are free again only after the caller's next barrier.
template <typename T>
__device__ __forceinline__ void row_argmax(const Ctx<T>& c, unsigned& bk, int& bi) {
    typedef RowT<T> R;
    bk = 0;
    bi = 0;
    for (int tile = c.wave; tile < c.ntiles; tile += S_NW) {
        const int v = tile * 64 + c.lane;
        if (v >= c.nvec) continue;
        unsigned raw[R::VEC];
        const unsigned m = c.load(v, raw);
#pragma unroll
        for (int e = 0; e < R::VEC; ++e) {
            const unsigned key = R::key(raw[e]);
            if ((m >> e & 1) && key > bk) { bk = key; bi = v * R::VEC + e - c.off; }  // (ascending i per thread)
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned ok = __shfl_xor(bk, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        if (ok > bk || (ok == bk && oi < bi)) { bk = ok; bi = oi; }
    }
    unsigned* wred = reinterpret_cast<unsigned*>(c.smem + L_WRED);
    if (c.lane == 0) { wred[c.wave] = bk; wred[S_NW + c.wave] = (unsigned)bi; }
    __syncthreads();
    bk = wred[0];
    bi = (int)wred[S_NW];
    for (int w = 1; w < S_NW; ++w) {
        const unsigned ok = wred[w];
        const int oi = (int)wred[S_NW + w];
        if (ok > bk || (ok == bk && oi < bi)) { bk = ok; bi = oi; }
    }
}

// Sum of weight(raw) over the row, in every thread.  Two barriers: L_MASS is free again on return.
template <typename T, typename WF>
__device__ __forceinline__ u64 row_total(const Ctx<T>& c, WF weight) {
    typedef RowT<T> R;
    u64* wsum = reinterpret_cast<u64*>(c.smem + L_MASS);
    u64 w = 0;
    for (int tile = c.wave; tile < c.ntiles; tile += S_NW) {
        const int v = tile * 64 + c.lane;
        if (v >= c.nvec) continue;
        unsigned raw[R::VEC];
        const unsigned m = c.load(v, raw);
#pragma unroll
        for (int e = 0; e < R::VEC; ++e)
            if (m >> e & 1) w += weight(raw[e]);
    }
    w = wave_sum64(w);
    if (c.lane == 0) wsum[c.wave] = w;
    __syncthreads();
    u64 t = 0;
    for (int i = 0; i < S_NW; ++i) t += wsum[i];
    __syncthreads();
    return t;
}

// Lowest index i at which the inclusive cumulative weight, in index order, exceeds the target; -1 when the total
// weight is 0.  W(raw, key, i) -> u64 weight; TF(total) -> target (< total).
template <typename T, typename WF, typename TF>
__device__ int prefix_find(const Ctx<T>& c, WF weight, TF target_of) {
    typedef RowT<T> R;
    u64* tsum = reinterpret_cast<u64*>(c.smem + L_MASS);
    u64* sc = c.scal();
    for (int tile = c.wave; tile < c.ntiles; tile += S_NW) {
        const int v = tile * 64 + c.lane;
        u64 w = 0;
        if (v < c.nvec) {
            unsigned raw[R::VEC];
            const unsigned m = c.load(v, raw);
#pragma unroll
            for (int e = 0; e < R::VEC; ++e)
                if (m >> e & 1) w += weight(raw[e], R::key(raw[e]), v * R::VEC + e - c.off);
        }
        w = wave_sum64(w);
        if (c.lane == 0) tsum[tile] = w;
    }
    __syncthreads();
    if (c.wave == 0) {
        // which tile: every lane sums a contiguous chunk of tiles
        const int chunk = (c.ntiles + 63) / 64;
        const int t0 = c.lane * chunk, t1 = min(t0 + chunk, c.ntiles);
        u64 t = 0;
        for (int i = t0; i < t1; ++i) t += tsum[i];
        const u64 incl = wave_scan64(t, c.lane);
        const u64 total = __shfl(incl, 63, 64);
        int result = -1;
        if (total > 0) {
            const u64 target = target_of(total);
            const u64 hit = __ballot(incl > target);
            const int first = hit ? __ffsll((long long)hit) - 1 : 63;
            u64 acc = incl - t;
            int tile = t0;
            if (c.lane == first) {
                for (; tile < t1 - 1; ++tile) {
                    if (acc + tsum[tile] > target) break;
                    acc += tsum[tile];
                }
            }
            tile = min(max(__shfl(tile, first, 64), 0), c.ntiles - 1);
            const u64 resid = target - __shfl(acc, first, 64);
            // which lane of that tile, then which element
            const int v = tile * 64 + c.lane;
            unsigned raw[R::VEC];
            u64 w[R::VEC], ws = 0;
            unsigned m = 0;
            if (v < c.nvec) m = c.load(v, raw);
#pragma unroll
            for (int e = 0; e < R::VEC; ++e) {
                w[e] = (m >> e & 1) ? weight(raw[e], R::key(raw[e]), v * R::VEC + e - c.off) : 0;
                ws += w[e];
            }
            const u64 li = wave_scan64(ws, c.lane);
            const u64 lhit = __ballot(li > resid);
            // (a lane always passes: the tile's sum is the same integers added again)
            const int lf = lhit ? __ffsll((long long)lhit) - 1 : 63;
            int idx = -1;
            if (c.lane == lf) {
                u64 a = li - ws;
#pragma unroll
                for (int e = 0; e < R::VEC; ++e) {
                    if (idx < 0 && w[e] > 0 && a + w[e] > resid) idx = v * R::VEC + e - c.off;
                    a += w[e];
                }
            }
            result = __shfl(idx, lf, 64);
        }
        if (c.lane == 0) sc[4] = (u64)(long long)result;
    }
    __syncthreads();
    const int res = (int)(long long)sc[4];
    __syncthreads();  // sc[4] and the tile sums are free again
    return res;
}

// the target of a draw with the uniform u among a total mass M: floor(u * M), below M
__device__ __forceinline__ u64 draw_target(float u, u64 M) {
    const u64 t = (u64)((double)u * (double)M);
    return t < M ? t : M - 1;  // u >= 1 (or its product rounding up to M): the last token with mass
}

// ---- the top-k / top-p cut (sample.hip's header comment, steps 2 and 3), shared by sample.hip and sample_rows.hip
// keep iff key > K, or key == K at an index <= I  (K = 0, I = V - 1: everything)
struct Filt {
    unsigned K;
    int I;
    __device__ __forceinline__ bool has(unsigned key, int i) const { return key > K || (key == K && i <= I); }
};

// One radix select inside the filter `in`.  MASS = false: the k-th key in rank order (target = k, on counts).
// MASS = true: the key at which the mass ranked before reaches P = ceil(top_p * Z), Z the mass inside `in`.
// Returns the key K and r: of the tokens inside `in` with key == K (n of them), the first r by index stay.
template <typename T, bool MASS>
__device__ void radix_select(const Ctx<T>& c, Filt in, u64 target, double top_p, unsigned& K, unsigned& r,
                             unsigned& n) {
    typedef RowT<T> R;
    unsigned* cnt = reinterpret_cast<unsigned*>(c.smem + L_CNT);
    u64* mass = reinterpret_cast<u64*>(c.smem + L_MASS);
    u64* sel = reinterpret_cast<u64*>(c.smem + L_SEL);
    unsigned* cntr = reinterpret_cast<unsigned*>(c.smem + L_CNTR);
    u64* sc = c.scal();
    unsigned prefix = 0;
    u64 above = 0;  // count / mass of the keys above the current prefix's range
    unsigned bincnt = 0;
    for (int level = 0; level < R::KB / 8; ++level) {
        const int shift = R::KB - 8 * (level + 1);
        for (int i = threadIdx.x; i < S_BINS * S_REP; i += S_NT) {
            cnt[i] = 0;
            if (MASS) mass[i] = 0;
        }
        __syncthreads();
        for (int tile = c.wave; tile < c.ntiles; tile += S_NW) {
            const int v = tile * 64 + c.lane;
            if (v >= c.nvec) continue;
            unsigned raw[R::VEC];
            const unsigned m = c.load(v, raw);
#pragma unroll
            for (int e = 0; e < R::VEC; ++e) {
                if (!(m >> e & 1)) continue;
                const unsigned key = R::key(raw[e]);
                if (!in.has(key, v * R::VEC + e - c.off)) continue;
                if (level > 0 && (key >> (shift + 8)) != prefix) continue;
                const int slot = (int)((key >> shift) & 255u) * S_REP + (c.lane & (S_REP - 1));
                atomicAdd(&cnt[slot], 1u);
                if (MASS) atomicAdd(&mass[slot], c.zq(raw[e]));
            }
        }
        __syncthreads();
        if (threadIdx.x < S_BINS) {  // sum the replicas, each thread starting at its own bank
            const int t = threadIdx.x;
            unsigned cc = 0;
            u64 mm = 0;
            for (int q = 0; q < S_REP; ++q) {
                const int s = t * S_REP + ((q + t) & (S_REP - 1));
                cc += cnt[s];
                if (MASS) mm += mass[s];
            }
            cntr[t] = cc;
            sel[t] = MASS ? mm : (u64)cc;
        }
        __syncthreads();
        if (c.wave == 0) {  // bins from 255 down, four per lane
            u64 s[4], t = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) { s[j] = sel[255 - 4 * c.lane - j]; t += s[j]; }
            const u64 incl = wave_scan64(t, c.lane);
            if (MASS && level == 0) {
                const u64 Z = __shfl(incl, 63, 64);
                u64 P = (u64)ceil(top_p * (double)Z);
                if (P > Z) P = Z;
                if (P < 1) P = 1;  // the first token in rank order always stays
                target = P;
            }
            const u64 need = target - above;
            const u64 hit = __ballot(incl >= need);
            // (no lane only on a row of NaNs, where Z = 0: take the lowest bin, which keeps everything)
            const int first = hit ? __ffsll((long long)hit) - 1 : 63;
            if (c.lane == first) {
                u64 acc = incl - t;
                int j = 0;
                for (; j < 3; ++j) {
                    if (acc + s[j] >= need) break;
                    acc += s[j];
                }
                const int bin = 255 - 4 * c.lane - j;
                sc[0] = (u64)bin;
                sc[1] = above + acc;
                sc[2] = (u64)cntr[bin];
                sc[3] = target;
            }
        }
        __syncthreads();
        prefix = (prefix << 8) | (unsigned)sc[0];
        above = sc[1];
        bincnt = (unsigned)sc[2];
        target = sc[3];
    }
    K = prefix;
    n = bincnt;
    if (!MASS) {
        r = (unsigned)(target - above);
    } else {
        // tie j (0-based, by index) of the n at K has above + j * zK ranked before it: it stays iff that is < P
        const u64 zk = (u64)(fminf(__expf((R::key_val(K) - c.xmax) * c.invT), 1.f) * S_FIX);
        const u64 rem = target > above ? target - above : 1;
        const u64 rr = zk ? (rem + zk - 1) / zk : (u64)n;
        r = (unsigned)(rr < (u64)n ? rr : (u64)n);
    }
    if (r < 1) r = 1;
    if (r > n) r = n;
}

// the index cutoff that keeps exactly the first r of the n tokens inside `in` with key == K
template <typename T>
__device__ Filt cut_ties(const Ctx<T>& c, Filt in, unsigned K, unsigned r, unsigned n) {
    int I = (K == in.K) ? in.I : c.V - 1;
    if (r < n) {
        const int i = prefix_find(
            c, [&](unsigned, unsigned key, int i) -> u64 { return (key == K && in.has(key, i)) ? 1 : 0; },
            [&](u64 total) -> u64 { const u64 t = r - 1; return t < total ? t : total - 1; });
        if (i >= 0) I = i;
    }
    return Filt{K, I};
}

// The token of one row: the argmax (T <= 0, and what every degenerate row falls back to: always inside [0, V)),
// else the draw at the uniform `u` among what top-k, top-p and min-p keep.  min_p > 0 keeps, of those, a token iff
// its fixed-point mass zq >= ceil(min_p * zq_max), zq_max the argmax's (2^40: the argmax always stays).
template <typename T>
__device__ int sample_row(Ctx<T>& c, float temperature, int top_k, double top_p, float min_p, float u) {
    typedef RowT<T> R;
    unsigned bk;
    int bi;
    row_argmax(c, bk, bi);
    int tok = bi;
    if (temperature > 0.f) {
        c.xmax = R::key_val(bk);
        c.invT = 1.f / temperature;
        Filt f{0u, c.V - 1};
        unsigned K, r, n;
        if (top_k > 0 && top_k < c.V) {
            radix_select<T, false>(c, f, (u64)top_k, 0.0, K, r, n);
            f = cut_ties(c, f, K, r, n);
        }
        if (top_p < 1.0) {
            radix_select<T, true>(c, f, 0, top_p, K, r, n);
            f = cut_ties(c, f, K, r, n);
        }
        u64 zmin = 0;
        if (min_p > 0.f) {
            const u64 zmax = c.zq(c.at(bi));
            zmin = (u64)ceil((double)min_p * (double)zmax);
            if (zmin > zmax) zmin = zmax;
        }
        const int i = prefix_find(
            c,
            [&](unsigned raw, unsigned key, int i) -> u64 {
                if (!f.has(key, i)) return 0;
                const u64 z = c.zq(raw);
                return z >= zmin ? z : 0;
            },
            [&](u64 M) -> u64 { return draw_target(u, M); });
        if (i >= 0 && i < c.V) tok = i;
    }
    return tok;
}

}  // namespace
}  // namespace bpe
