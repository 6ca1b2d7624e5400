// Speculative-decoding verification for gfx950: one 1024-thread workgroup per sequence decides how many of its K
// draft tokens stand and draws the token after them (ops/sampling.py states the function; tests/spec_refs.py is its
// fp64 oracle).  No global atomics, no inter-workgroup traffic; every loop is bounded by K or V.
//
//   greedy:   n = leading i with d[i] == argmax t[i-1];  y = argmax t[n].
//   sampling: p_i = softmax(t[i-1] / T), q_i = softmax(s[i] / T); draft i stands iff ua[i] * q_i(d[i]) < p_i(d[i]);
//             after the first rejection y is drawn from max(p - q, 0) of that position (from p when that is all
//             zero), after K acceptances from p_{K+1}; both draws are the index-order inverse CDF at us.
//
// How: the accept tests run in order and stop at the first rejection -- the decision is computed from LDS
// broadcasts and one element per row, so it is uniform over the workgroup -- and only the rows up to there are
// normalised: per row an argmax pass (the max) and a mass pass, over 16-byte vectors as in sample.hip
// (sample_common.h).  Masses are 2^-40 fixed point, so Z_p, Z_q and the residual sums are order-independent
// integers and the kernel is a pure function of its inputs.  The accept test is cross-multiplied,
// ua * zq(d) * Z_p < zp(d) * Z_q, in fp64 (exact to 2^-52 on integers below 2^57).  The residual weight of token j
// is floor(max(zp_j / Z_p - zq_j / Z_q, 0) * 2^40), a function of integers only; its p row is read in vectors, its
// q row element by element at the same index (the two rows need not share an alignment).
//
// point_mass (prompt-lookup drafts: q_i is the point mass at d[i], there are no draft logits): the q row passes are
// skipped and zq(d) = Z_q = 2^40, zq elsewhere = 0 stand in the same expressions, which is what one-hot draft logits
// (0 at d[i], -inf elsewhere) give the code above, bit for bit.  A d outside [0, V) never stands and is never read;
// the token after it is drawn from p itself.
//
// All writes are plain vector stores by thread 0.
#include "sample_common.h"

namespace bpe {
namespace {

template <typename T>
__global__ void __launch_bounds__(S_NT) spec_verify_kernel(SpecArgs a) {
    typedef RowT<T> R;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int b = blockIdx.x;
    const int K = a.K, V = a.V;
    if (a.n_out != nullptr && (a.done[b] != 0 || a.step_t[b] == 0)) return;  // an idle row: nothing at all
    const long long* draft = a.draft + (long)b * a.draft_ld;

    u64 seed = 0, cnt = 0;
    if (a.rng != nullptr) { seed = (u64)a.rng[0]; cnt = (u64)a.rng[1]; }

    Ctx<T> cp, cq;
    unsigned bk;
    int bi, n = 0, y;
    if (!(a.temperature > 0.f) || (a.s == nullptr && !a.point_mass)) {
        for (n = 0;; ++n) {
            cp.init(a.t, (long)b * (K + 1) + n, V, smem);
            row_argmax(cp, bk, bi);
            __syncthreads();
            if (n == K || draft[n] != (long long)bi) break;
        }
        y = bi;
    } else {
        const float invT = 1.f / a.temperature;
        u64 Zp = 0, Zq = 0;
        for (n = 0; n < K; ++n) {
            cp.init(a.t, (long)b * (K + 1) + n, V, smem);
            cp.invT = invT;
            row_argmax(cp, bk, bi);
            cp.xmax = R::key_val(bk);
            Zp = row_total(cp, [&](unsigned raw) -> u64 { return cp.zq(raw); });
            if (!a.point_mass) {
                cq.init(a.s, (long)b * K + n, V, smem);
                cq.invT = invT;
                unsigned qk;
                int qi;
                row_argmax(cq, qk, qi);
                cq.xmax = R::key_val(qk);
                Zq = row_total(cq, [&](unsigned raw) -> u64 { return cq.zq(raw); });
            } else {
                Zq = (u64)S_FIX;
            }
            const long long d = draft[n];
            bool ok = false;
            if (d >= 0 && d < V) {  // (a token outside the vocabulary is never read and never stands)
                const float ua = a.rng != nullptr ? philox_u(seed, cnt + (u64)n, (unsigned)b, 1u) : a.ua[(long)b * K + n];
                const u64 zqd = a.point_mass ? (u64)S_FIX : cq.zq(cq.at((int)d));
                const double lhs = (double)ua * (double)zqd * (double)Zp;
                const double rhs = (double)cp.zq(cp.at((int)d)) * (double)Zq;
                ok = lhs < rhs;
            }
            if (!ok) break;
        }
        const float us = a.rng != nullptr ? philox_u(seed, cnt, (unsigned)b, 2u) : a.us[b];
        int i = -1;
        if (n < K && a.point_mass) {  // rejected at position n + 1: p with d zeroed (a d outside [0, V): p itself)
            const long long d = draft[n];
            const double ip = Zp ? 1.0 / (double)Zp : 0.0, iq = 1.0 / (double)S_FIX;
            if (d >= 0 && d < V)
                i = prefix_find(
                    cp,
                    [&](unsigned raw, unsigned, int j) -> u64 {
                        const double r = (double)cp.zq(raw) * ip - (double)(j == (int)d ? (u64)S_FIX : (u64)0) * iq;
                        return r > 0.0 ? (u64)(r * (double)S_FIX) : 0;
                    },
                    [&](u64 M) -> u64 { return draw_target(us, M); });
        } else if (n < K) {  // rejected at position n + 1: the residual of that position (cp, cq, Zp, Zq are its own)
            const double ip = Zp ? 1.0 / (double)Zp : 0.0, iq = Zq ? 1.0 / (double)Zq : 0.0;
            i = prefix_find(
                cp,
                [&](unsigned raw, unsigned, int j) -> u64 {
                    const double r = (double)cp.zq(raw) * ip - (double)cq.zq(cq.at(j)) * iq;
                    return r > 0.0 ? (u64)(r * (double)S_FIX) : 0;
                },
                [&](u64 M) -> u64 { return draw_target(us, M); });
        } else {
            cp.init(a.t, (long)b * (K + 1) + K, V, smem);
            cp.invT = invT;
            row_argmax(cp, bk, bi);
            cp.xmax = R::key_val(bk);
            __syncthreads();
        }
        if (i < 0)  // all K stand, or no residual mass: from p
            i = prefix_find(cp, [&](unsigned raw, unsigned, int) -> u64 { return cp.zq(raw); },
                            [&](u64 M) -> u64 { return draw_target(us, M); });
        y = (i >= 0 && i < V) ? i : bi;  // (a row without mass falls back to its argmax: always inside [0, V))
    }

    if (threadIdx.x != 0) return;
    if (a.n_out == nullptr) {
        a.res_n[b] = n;
        a.res_y[b] = y;
        return;
    }
    const int o = a.n_out[b];
    int m = 0;
    bool fin = false;
    long long last = 0;
    for (int j = 0; j <= n && !fin; ++j) {
        if (o + m >= a.out_n) break;
        last = j < n ? draft[j] : (long long)y;
        a.out[(long)b * a.out_ld + o + m] = last;
        ++m;
        fin = a.eos >= 0 && last == (long long)a.eos;
    }
    fin = fin || o + m >= a.out_n;
    a.n_out[b] = o + m;
    if (m > 0) {
        a.win[(long)b * a.win_ld] = last;
        a.ids[b] = last;
        a.pos_t[b] = a.base[b] + m;
        a.pos_d[b] = a.base[b] + m;
    }
    if (fin) {
        a.done[b] = 1;
        a.step_t[b] = 0;
        a.step_d[b] = 0;
    }
}

}  // namespace
}  // namespace bpe

using namespace bpe;

void launch_spec_verify(const SpecArgs& a, int dtype, int B, hipStream_t s) {
    if (B == 0) return;
    if (dtype == DT_BF16) {
        hipFuncSetAttribute(reinterpret_cast<const void*>(&spec_verify_kernel<__bf16>),
                            hipFuncAttributeMaxDynamicSharedMemorySize, L_TOTAL);
        spec_verify_kernel<__bf16><<<B, S_NT, L_TOTAL, s>>>(a);
    } else {
        hipFuncSetAttribute(reinterpret_cast<const void*>(&spec_verify_kernel<float>),
                            hipFuncAttributeMaxDynamicSharedMemorySize, L_TOTAL);
        spec_verify_kernel<float><<<B, S_NT, L_TOTAL, s>>>(a);
    }
}
