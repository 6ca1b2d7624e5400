// Token sampling (greedy / temperature / top-k / top-p) for gfx950: one 1024-thread workgroup per logits row, no
// sort, no global atomics, no inter-workgroup traffic; every loop is bounded by V.
//
// The function (ops/sampling.py states it in full; tests/sample_refs.py is its fp64 oracle):
//   z_i = exp((x_i - max x) / T); rank order = descending x, ascending index among equal x; top-k keeps the first
//   min(k, V) in rank order; top-p keeps, of those, a token iff the mass ranked strictly before it is < top_p * Z;
//   the draw is the lowest kept index whose inclusive kept mass in index order exceeds u * M.
//
// How: the row ([V] bf16 or fp32, just written by the LM head, L2-resident) is re-read per pass rather than staged
// (an fp32 row of 50257 does not fit the LDS, and one code path serves both types).  A row start is only
// element-aligned (V = 50257 is odd), so the row is addressed in "virtual" 16-byte vectors that ARE aligned: virtual
// element j = i + off with off = the row start's offset inside its 16-byte granule.  Interior vectors are one
// 16-byte load; the head and tail vectors are loaded element by element under a validity mask, so nothing outside
// [0, V) is ever touched.  Thread-tile = one vector, wave-tile = 64 vectors; wave w takes tiles w, w + 16, ...
//
//   1. argmax pass: max of the order-preserving key (sign-flipped bits, -0 folded into +0), lowest index on ties.
//   2. top-k: radix select on the key, 8 bits per level (2 levels bf16, 4 fp32) over a count histogram.
//   3. top-p: the same select over a mass histogram of what top-k kept.
//      Both leave (K, r): keep key > K and the first r tokens, by index, with key == K; the index of the r-th such
//      token (found only when r cuts a run of equal values) turns the filter into key > K || (key == K && i <= I).
//   4. draw: per-tile kept mass -> the tile, lane and element at which the cumulative mass passes u * M.
//
// Masses are 64-bit fixed point (z * 2^40, z <= 1): integer sums do not depend on the order of the adds, so the
// histograms (LDS atomics) and the cumulative sums give the same bits every run, and the error against exact z is
// V * 2^-41 of the mass of the top token -- below the fp32 exp's own.  Histogram bins are replicated 32x, replica
// = lane % 32, at address bin * 32 + replica: every lane of a half-wave lands in its own LDS bank whatever the bins
// are, so equal logits (most of a row shares a few exponent bins) never serialise the atomics.
//
// The row addressing, Philox, the argmax, the order-independent sums and the index-order draw live in
// sample_common.h, which spec_verify.hip shares.
#include "sample_common.h"

namespace bpe {
namespace {

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

template <typename T>
__global__ void __launch_bounds__(S_NT) sample_kernel(SampleArgs a) {
    typedef RowT<T> R;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int row = blockIdx.x;
    Ctx<T> c;
    c.init(a.logits, (long)row, a.V, smem);

    // ---- argmax: highest key, lowest index among equals
    unsigned bk;
    int bi;
    row_argmax(c, bk, bi);
    int tok = bi;  // greedy, and what every degenerate row (all NaN, no mass) falls back to: always inside [0, V)

    // ---- the uniform: given, or Philox4x32-10 keyed by the seed at counter (count, row, 0)
    long long count = 0;
    float u = 0.5f;
    if (a.rng != nullptr) {
        const u64 seed = (u64)a.rng[0];
        count = a.rng[1];
        u = philox_u(seed, (u64)count, (unsigned)row, 0u);
    } else if (a.u != nullptr) {
        u = a.u[row];
    }

    if (a.temperature > 0.f) {
        c.xmax = R::key_val(bk);
        c.invT = 1.f / a.temperature;
        Filt f{0u, a.V - 1};
        unsigned K, r, n;
        if (a.top_k > 0 && a.top_k < a.V) {
            radix_select<T, false>(c, f, (u64)a.top_k, 0.0, K, r, n);
            f = cut_ties(c, f, K, r, n);
        }
        if (a.top_p < 1.0) {
            radix_select<T, true>(c, f, 0, a.top_p, K, r, n);
            f = cut_ties(c, f, K, r, n);
        }
        const int i = prefix_find(
            c, [&](unsigned raw, unsigned key, int i) -> u64 { return f.has(key, i) ? c.zq(raw) : 0; },
            [&](u64 M) -> u64 { return draw_target(u, M); });
        if (i >= 0 && i < a.V) tok = i;
    }

    if (threadIdx.x == 0) {
        if (a.res != nullptr) a.res[row] = tok;
        if (a.ids != nullptr) {
            const bool idle = a.done[row] != 0 || (a.step != nullptr && a.step[row] == 0);
            a.ids[row] = tok;
            if (a.col >= 0) {  // a named column (a speculative window): an idle row leaves it as it is
                if (a.col < a.out_n && !idle) a.out[(long)row * a.out_ld + a.col] = (long long)tok;
            } else if (count >= 0 && count < a.out_n) {
                a.out[(long)row * a.out_ld + count] = idle ? -1 : (long long)tok;
            }
            if (!idle && a.eos >= 0 && tok == a.eos) {
                a.done[row] = 1;
                if (a.step != nullptr) a.step[row] = 0;
            }
        }
    }
}

}  // namespace
}  // namespace bpe

using namespace bpe;

void launch_sample(const SampleArgs& a, int dtype, int B, hipStream_t s) {
    if (B == 0) return;
    if (dtype == DT_BF16) {
        hipFuncSetAttribute(reinterpret_cast<const void*>(&sample_kernel<__bf16>),
                            hipFuncAttributeMaxDynamicSharedMemorySize, L_TOTAL);
        sample_kernel<__bf16><<<B, S_NT, L_TOTAL, s>>>(a);
    } else {
        hipFuncSetAttribute(reinterpret_cast<const void*>(&sample_kernel<float>),
                            hipFuncAttributeMaxDynamicSharedMemorySize, L_TOTAL);
        sample_kernel<float><<<B, S_NT, L_TOTAL, s>>>(a);
    }
}
