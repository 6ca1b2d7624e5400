// Prompt-lookup (n-gram) drafts for gfx950: one 256-thread workgroup per sequence finds the most recent earlier
// occurrence of the longest suffix (n_lo .. n_hi tokens) of the sequence's own history and proposes what followed
// it (ops/sampling.py states the function; tests/lookup_refs.py is its brute-force oracle).  No global atomics, no
// inter-workgroup traffic; every loop is bounded by L, n_hi or K.
//
//   history   h = prompt[b][0 .. n_prompt[b]) ++ out[b][0 .. n_out[b]), L tokens; never materialised in global memory.
//   candidate an end position e, 0 <= e <= L - 2; m(e) = the number of leading j < min(n_hi, e + 1) with
//             h[e - j] == h[L - 1 - j].  The best is the largest (m, e); it is a match iff m >= n_lo.
//   drafts    match: d[j] = h[e + 1 + j mod (L - 1 - e)];  none: d[j] = h[L - 1].
//
// How: the int64 ids are staged once into LDS as int32 while L <= LK_STAGE (a compare then reads consecutive
// dwords across the lanes and one broadcast dword); a longer history is scanned in global memory by the same code.
// Each thread walks the candidates e = tid, tid + 256, ... and keeps the largest key (m << 32 | e); a wave
// shuffle reduction and four LDS words give the workgroup's maximum.  Keys of different candidates differ, so the
// maximum does not depend on the order of the compares and the kernel is a pure function of its inputs.
//
// All writes are plain vector stores to win[b][1 .. K].
#include "common.h"
#include "kernels.h"

namespace bpe {
namespace {

typedef unsigned long long u64;

constexpr int LK_NT = 256, LK_NW = LK_NT / 64;
constexpr int LK_STAGE = 8192;  // tokens staged in LDS (32 KiB)

template <bool STAGED>
__device__ __forceinline__ void lookup_row(const LookupArgs& a, const long long* pr, const long long* po, int np, int L,
                                           long long* win, int* hs, u64* wred) {
    const int tid = threadIdx.x;
    auto h = [&](int i) -> int {  // 0 <= i < L
        if constexpr (STAGED) return hs[i];
        return (int)(i < np ? pr[i] : po[i - np]);
    };
    if constexpr (STAGED) {
        for (int i = tid; i < L; i += LK_NT) hs[i] = (int)(i < np ? pr[i] : po[i - np]);
        __syncthreads();
    }
    u64 best = 0;  // (m << 32) | e; 0: no candidate matches even one token
    for (int e = tid; e <= L - 2; e += LK_NT) {  // (ascending e per thread: a later equal m replaces an earlier)
        const int tmax = min(a.n_hi, e + 1);
        int t = 0;
        while (t < tmax && h(e - t) == h(L - 1 - t)) ++t;
        if (t > 0) {
            const u64 key = ((u64)t << 32) | (unsigned)e;
            best = key > best ? key : best;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const u64 other = __shfl_xor(best, o, 64);
        best = other > best ? other : best;
    }
    if ((tid & 63) == 0) wred[tid >> 6] = best;
    __syncthreads();
    best = wred[0];
#pragma unroll
    for (int w = 1; w < LK_NW; ++w) best = wred[w] > best ? wred[w] : best;

    const int m = (int)(best >> 32), e = (int)(unsigned)best;
    const bool hit = m >= a.n_lo;  // (n_lo >= 1, so best == 0 is never a hit)
    const int p = hit ? L - 1 - e : 1, from = hit ? e + 1 : L - 1;
    for (int j = tid; j < a.K; j += LK_NT) win[1 + j] = (long long)h(from + j % p);
}

__global__ void __launch_bounds__(LK_NT) lookup_draft_kernel(LookupArgs a) {
    __shared__ int hs[LK_STAGE];
    __shared__ u64 wred[LK_NW];
    const int b = blockIdx.x;
    if (a.done[b] != 0 || a.step[b] == 0) return;  // an idle row: nothing at all
    const int np = min(max(a.n_prompt[b], 0), a.prompt_n), no = min(max(a.n_out[b], 0), a.out_n);
    const int L = np + no;
    if (L < 1) return;  // (no history, no last token: nothing to propose)
    const long long* pr = a.prompt + (long)b * a.prompt_ld;
    const long long* po = a.out + (long)b * a.out_ld;
    long long* win = a.win + (long)b * a.win_ld;
    if (L <= LK_STAGE)  // (uniform over the workgroup)
        lookup_row<true>(a, pr, po, np, L, win, hs, wred);
    else
        lookup_row<false>(a, pr, po, np, L, win, hs, wred);
}

}  // namespace
}  // namespace bpe

using namespace bpe;

void launch_lookup_draft(const LookupArgs& a, int B, hipStream_t s) {
    if (B == 0 || a.K == 0) return;
    lookup_draft_kernel<<<B, LK_NT, 0, s>>>(a);
}
