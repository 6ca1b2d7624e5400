// Sampling controls for gfx950: logit bias, repetition / presence / frequency penalties and the row's log-sum-exp in
// one pass over a logits row (logit_process_kernel), and the per-sequence token history + the emitted token's
// log-probability (token_commit_kernel).  No global atomics, no inter-workgroup traffic; every loop is bounded by V.
//
// The function (ops/sampling.py states it in full; tests/logit_refs.py is its fp64 oracle):
//   hist[b][v] = 2 * (times v was emitted) + (v occurs in the prompt);  seen = hist != 0, c = hist >> 1
//   y = x + bias[v];  seen: y = y > 0 ? y * (1 / rp) : y * rp;  y = y - fp * c - pp * (c > 0);  out = round(y)
//   lse[b] = max x + log(sum exp(x - max x)) over the UNPROCESSED row, fp32 max and fp32 sum
//   token_commit: tok = tokens[b][count] >= 0:  hist[b][tok] += 2,  logprob[b][count] = float(raw[b][tok]) - lse[b]
//
// logit_process_kernel<T>: one 1024-thread workgroup per row, the row ([V] bf16 or fp32, just written by the LM head,
// L2-resident) addressed through sample_common.h's Ctx: virtual 16-byte vectors that ARE aligned, the unaligned head
// and the tail loaded element by element under a validity mask, nothing outside [0, V) touched.  Passes:
//   1. (lse only) max of the row: per thread, wave shuffles, then 16 partials through the LDS;
//   2. (lse only) sum of exp(x - max), the same way.  The partials are combined in one fixed order by every thread,
//      so the result has the same bits every run;
//   3. (out only) the element arithmetic.  hist and bias are indexed by the real element index with plain 4-byte
//      loads.  An element with hist == 0 and bias == 0 (or none) keeps its input BITS: no arithmetic touches it, so
//      -0.0 stays -0.0.  The output row has its own element offset; when it equals the input's, interior vectors are
//      one 16-byte store, otherwise (and for the head and tail) element stores under the same mask.
// In place (out == x) is safe: pass 3 starts after the barrier that ends pass 2, every thread then reads and writes
// its own vectors only, and without lse there is no other reader.
//
// token_commit_kernel: one thread per row, plain vector load / add / store on hist (no two rows share an address).
//
// logit_process_rows_kernel / token_commit_rows_kernel (continuous batching): the same two row bodies with rp,
// 1 / rp, pp, fp read from fp32 [B] tables, an optional rows map (launched row r -> slot b) and the column taken
// from a per-slot counter; an idle slot (done, or step == 0) writes nothing.
//
// Resources (hipcc -O3, gfx950, -Rpass-analysis=kernel-resource-usage), no scratch in any of them:
//   logit_process_kernel<__bf16>: 32 VGPRs, 62 SGPRs, 128 B LDS, occupancy 8 waves / SIMD
//   logit_process_kernel<float>:  30 VGPRs, 52 SGPRs, 128 B LDS, occupancy 8 waves / SIMD
//   token_commit_kernel:           8 VGPRs, 22 SGPRs, 0 LDS
//   logit_process_rows_kernel: as logit_process_kernel of the same type; token_commit_rows_kernel: 12 VGPRs, 22 SGPRs
#include "sample_common.h"

namespace bpe {
namespace {

__device__ __forceinline__ unsigned to_raw(float y, __bf16*) { return f2bf(y); }
__device__ __forceinline__ unsigned to_raw(float y, float*) { return __float_as_uint(y); }

// max / sum of one value per thread over the workgroup, in every thread: wave shuffles, then the 16 wave partials
// through `red`, combined in index order.  One barrier; `red` is free again after the caller's next barrier.
template <bool MAX>
__device__ __forceinline__ float block_reduce(float v, float* red, int lane, int wave) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float t = __shfl_xor(v, o, 64);
        v = MAX ? fmaxf(v, t) : v + t;
    }
    if (lane == 0) red[wave] = v;
    __syncthreads();
    float r = red[0];
#pragma unroll
    for (int w = 1; w < S_NW; ++w) r = MAX ? fmaxf(r, red[w]) : r + red[w];
    return r;
}

// One row: x / out row `row`, hist / lse row `slot` (the same number for logit_process_kernel), with the penalty
// values of `a`.
template <typename T>
__device__ __forceinline__ void logit_process_row(const LogitArgs& a, int row, int slot, float (&red)[2][S_NW]) {
    typedef RowT<T> R;
    typedef typename R::raw_t raw_t;
    Ctx<T> c;
    c.init(a.x, (long)row, a.V, reinterpret_cast<char*>(&red[0][0]));

    if (a.lse != nullptr) {
        const float NINF = -__builtin_inff();
        float m = NINF;
        for (int tile = c.wave; tile < c.ntiles; tile += S_NW) {
            const int v = tile * 64 + c.lane;
            if (v >= c.nvec) continue;
            unsigned raw[R::VEC];
            const unsigned msk = c.load(v, raw);
#pragma unroll
            for (int e = 0; e < R::VEC; ++e)
                if (msk >> e & 1) m = fmaxf(m, R::val(raw[e]));
        }
        m = block_reduce<true>(m, red[0], c.lane, c.wave);
        float s = 0.f;
        if (m > NINF) {  // (a row of -inf has no mass: lse = -inf)
            for (int tile = c.wave; tile < c.ntiles; tile += S_NW) {
                const int v = tile * 64 + c.lane;
                if (v >= c.nvec) continue;
                unsigned raw[R::VEC];
                const unsigned msk = c.load(v, raw);
#pragma unroll
                for (int e = 0; e < R::VEC; ++e)
                    if (msk >> e & 1) s += __expf(R::val(raw[e]) - m);  // exp(-inf) = 0
            }
        }
        s = block_reduce<false>(s, red[1], c.lane, c.wave);  // its barrier: every read of x is done
        if (threadIdx.x == 0) a.lse[slot] = m > NINF ? m + logf(s) : NINF;
    }

    if (a.out == nullptr) return;
    raw_t* orow = reinterpret_cast<raw_t*>(a.out) + (long)row * a.V;
    const int ooff = (int)((reinterpret_cast<uintptr_t>(orow) / sizeof(raw_t)) % R::VEC);
    const bool same = ooff == c.off;  // then virtual vector v of the output row is aligned too
    const int* hrow = a.hist != nullptr ? a.hist + (long)slot * a.V : nullptr;
    const unsigned FULL = (1u << R::VEC) - 1;
    for (int tile = c.wave; tile < c.ntiles; tile += S_NW) {
        const int v = tile * 64 + c.lane;
        if (v >= c.nvec) continue;
        unsigned raw[R::VEC];
        const unsigned msk = c.load(v, raw);
        const int i0 = v * R::VEC - c.off;
#pragma unroll
        for (int e = 0; e < R::VEC; ++e) {
            if (!(msk >> e & 1)) continue;
            const int i = i0 + e;  // inside [0, V)
            const int h = hrow != nullptr ? hrow[i] : 0;
            const float b = a.bias != nullptr ? a.bias[i] : 0.f;
            if (h == 0 && b == 0.f) continue;  // untouched: the input's bits
            float y = R::val(raw[e]);
            if (a.bias != nullptr) y = y + b;
            if (h != 0) {
                y = y > 0.f ? y * a.inv_rp : y * a.rp;
                const int cnt = h >> 1;
                if (cnt > 0) y = y - a.fp * (float)cnt - a.pp;
            }
            raw[e] = to_raw(y, (T*)nullptr);
        }
        if (same && msk == FULL) {
            if constexpr (R::VEC == 8) {
                u16x8 t;
#pragma unroll
                for (int e = 0; e < 8; ++e) t[e] = (u16)raw[e];
                *reinterpret_cast<u16x8*>(orow + i0) = t;
            } else {
                typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
                u32x4 t;
#pragma unroll
                for (int e = 0; e < 4; ++e) t[e] = raw[e];
                *reinterpret_cast<u32x4*>(orow + i0) = t;
            }
        } else {
#pragma unroll
            for (int e = 0; e < R::VEC; ++e)
                if (msk >> e & 1) orow[i0 + e] = (raw_t)raw[e];
        }
    }
}

template <typename T>
__global__ void __launch_bounds__(S_NT) logit_process_kernel(LogitArgs a) {
    __shared__ float red[2][S_NW];
    logit_process_row<T>(a, blockIdx.x, blockIdx.x, red);
}

// logit_process with the penalty values read per slot: launched row r is slot b = rows[r] (nullptr: r).  A slot that
// is done or whose step is 0 writes nothing; a slot whose penalties are all neutral (rp = 1, pp = fp = 0) runs
// without the history, so that only a bias touches its row.
template <typename T>
__global__ void __launch_bounds__(S_NT) logit_process_rows_kernel(LogitRowsArgs ra) {
    __shared__ float red[2][S_NW];
    const int r = blockIdx.x;
    const int b = ra.rows != nullptr ? ra.rows[r] : r;
    if (b < 0 || b >= ra.B) return;
    if (ra.done[b] != 0 || ra.step[b] == 0) return;  // (the whole workgroup: no barrier is left behind)
    LogitArgs a = ra.a;
    if (a.hist != nullptr) {
        a.rp = ra.rp[b];
        a.inv_rp = ra.inv_rp[b];
        a.pp = ra.pp[b];
        a.fp = ra.fp[b];
        if (a.rp == 1.f && a.pp == 0.f && a.fp == 0.f) a.hist = nullptr;
    }
    logit_process_row<T>(a, r, b, red);
}

// the body of both commit kernels: column `col` of row `row` of tokens / logprob, row `row` of raw, row `slot` of
// hist and lse
__device__ __forceinline__ void token_commit_row(const CommitArgs& a, int row, int slot, long long count) {
    if (count < 0 || count >= a.tok_n) return;
    const long long tok = a.tokens[(long)slot * a.tok_ld + count];
    if (tok < 0 || tok >= a.V) return;  // -1: an idle row
    if (a.hist != nullptr) {
        int* h = a.hist + (long)slot * a.V + tok;
        *h = *h + 2;
    }
    if (a.logprob != nullptr && count < a.lp_n) {
        const long i = (long)row * a.V + tok;
        const float x = a.dtype == DT_BF16 ? bf2f(reinterpret_cast<const u16*>(a.raw)[i])
                                           : reinterpret_cast<const float*>(a.raw)[i];
        a.logprob[(long)slot * a.lp_ld + count] = x - a.lse[slot];
    }
}

// token_commit on a per-slot counter: slot b = rows[r] commits column count[b] - 1 iff count[b] has moved past
// committed[b] -- the sampler emitted since the last commit -- and then sets committed[b] = count[b].
__global__ void __launch_bounds__(256) token_commit_rows_kernel(CommitRowsArgs ra, int R) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= R) return;
    const int b = ra.rows != nullptr ? ra.rows[r] : r;
    if (b < 0 || b >= ra.B) return;
    const long long n = ra.count[b];
    if (n <= ra.committed[b]) return;
    ra.committed[b] = n;
    token_commit_row(ra.a, r, b, n - 1);
}

__global__ void __launch_bounds__(256) token_commit_kernel(CommitArgs a, int B) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    token_commit_row(a, b, b, a.rng[1]);
}

}  // namespace
}  // namespace bpe

using namespace bpe;

void launch_logit_process(const LogitArgs& a, int dtype, int B, hipStream_t s) {
    if (B == 0 || (a.out == nullptr && a.lse == nullptr)) return;
    if (dtype == DT_BF16) logit_process_kernel<__bf16><<<B, S_NT, 0, s>>>(a);
    else logit_process_kernel<float><<<B, S_NT, 0, s>>>(a);
}

void launch_token_commit(const CommitArgs& a, int B, hipStream_t s) {
    if (B == 0 || (a.hist == nullptr && a.logprob == nullptr)) return;
    token_commit_kernel<<<(B + 255) / 256, 256, 0, s>>>(a, B);
}

void launch_logit_process_rows(const LogitRowsArgs& a, int dtype, int R, hipStream_t s) {
    if (R == 0 || (a.a.out == nullptr && a.a.lse == nullptr)) return;
    if (dtype == DT_BF16) logit_process_rows_kernel<__bf16><<<R, S_NT, 0, s>>>(a);
    else logit_process_rows_kernel<float><<<R, S_NT, 0, s>>>(a);
}

void launch_token_commit_rows(const CommitRowsArgs& a, int R, hipStream_t s) {
    if (R == 0 || (a.a.hist == nullptr && a.a.logprob == nullptr)) return;
    token_commit_rows_kernel<<<(R + 255) / 256, 256, 0, s>>>(a, R);
}
