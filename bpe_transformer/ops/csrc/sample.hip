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
// sample_common.h, which spec_verify.hip shares; so do the radix select, the tie cut and the row's whole draw (Filt,
// radix_select, cut_ties, sample_row), which sample_rows.hip -- this kernel with every parameter read per row --
// shares: this kernel is sample_row with min_p = 0 plus the scalar epilogue.
#include "sample_common.h"

namespace bpe {
namespace {

template <typename T>
__global__ void __launch_bounds__(S_NT) sample_kernel(SampleArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int row = blockIdx.x;
    Ctx<T> c;
    c.init(a.logits, (long)row, a.V, smem);

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

    // ---- the token (sample_common.h): steps 1-4 of the header; min_p = 0 keeps every mass z >= 0
    const int tok = sample_row(c, a.temperature, a.top_k, a.top_p, 0.f, u);

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
