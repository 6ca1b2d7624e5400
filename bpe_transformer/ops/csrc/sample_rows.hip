// Per-row token sampling for continuous batching on gfx950: sample.hip's algorithm (one 1024-thread workgroup per
// launched logits row, no sort, no global atomics, every loop bounded by V) with every parameter read from per-slot
// device tables, so that requests with different sampling parameters, seeds and lengths share one captured graph.
//
// The function (ops/sampling.py states it in full; tests/sample_rows_refs.py is its fp64 oracle).  Launched row r is
// slot b = rows[r] (no map: b = r).  The logits are row r of [R][V]; everything else is indexed by b:
//   * idle: done[b] != 0 or step[b] == 0 -> the workgroup returns before its first barrier and writes nothing;
//   * u = u[r] if given, else Philox4x32-10 keyed by seed[b] at counter (count[b], philox_row[b], 0): the row word
//     comes from the table, not from the slot.  0 (a served request) makes the stream depend on neither the slot nor
//     its neighbours; philox_row[b] = b with one seed for all slots is sample.hip's stream (generate);
//   * token = sample.hip's draw with temperature[b], top_k[b], top_p[b] (fp64, as the scalar kernel's ceil(top_p * Z)
//     is computed in double) and, new here, min_p[b]: of what top-k and top-p kept, a token stays iff its fixed-point
//     mass zq >= ceil(min_p * zq_max); zq_max = 2^40 is the argmax's, so the argmax always stays (sample_row,
//     sample_common.h);
//   * ids[b] = out[b][count[b]] = token; count[b] += 1; token == eos[b] or count[b] >= limit[b]: done[b] = 1,
//     step[b] = 0.  The kernel advances the counter itself: no second launch.
// All of it is written by thread 0 with plain C++ stores (no two slots share an address; a rows map names a slot
// at most once).
//
// Resources (hipcc -O3, gfx950, -Rpass-analysis=kernel-resource-usage): 128 VGPRs, 90 (bf16) / 91 (fp32) SGPRs, no
// scratch, occupancy 4 waves / SIMD; the dynamic LDS of sample_kernel (L_TOTAL).
#include "sample_common.h"

namespace bpe {
namespace {

template <typename T>
__global__ void __launch_bounds__(S_NT) sample_rows_kernel(SampleRowsArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int r = blockIdx.x;
    const int b = a.rows != nullptr ? a.rows[r] : r;
    if (b < 0 || b >= a.B) return;
    if (a.done[b] != 0 || a.step[b] == 0) return;  // idle (uniform over the workgroup)
    Ctx<T> c;
    c.init(a.logits, (long)r, a.V, smem);

    const long long count = a.count[b];
    const float u = a.u != nullptr ? a.u[r] : philox_u((u64)a.seed[b], (u64)count, (unsigned)a.philox_row[b], 0u);
    int top_k = a.top_k[b];
    if (top_k > a.V) top_k = a.V;
    const int tok = sample_row(c, a.temperature[b], top_k, a.top_p[b], a.min_p[b], u);

    if (threadIdx.x == 0) {
        a.ids[b] = (long long)tok;
        if (count >= 0 && count < a.out_n) a.out[(long)b * a.out_ld + count] = (long long)tok;
        const long long next = count + 1;
        a.count[b] = next;
        const int eos = a.eos[b];
        if ((eos >= 0 && tok == eos) || next >= (long long)a.limit[b]) {
            a.done[b] = 1;
            a.step[b] = 0;
        }
    }
}

}  // namespace
}  // namespace bpe

using namespace bpe;

void launch_sample_rows(const SampleRowsArgs& a, int dtype, int R, hipStream_t s) {
    if (R == 0) return;
    if (dtype == DT_BF16) {
        hipFuncSetAttribute(reinterpret_cast<const void*>(&sample_rows_kernel<__bf16>),
                            hipFuncAttributeMaxDynamicSharedMemorySize, L_TOTAL);
        sample_rows_kernel<__bf16><<<R, S_NT, L_TOTAL, s>>>(a);
    } else {
        hipFuncSetAttribute(reinterpret_cast<const void*>(&sample_rows_kernel<float>),
                            hipFuncAttributeMaxDynamicSharedMemorySize, L_TOTAL);
        sample_rows_kernel<float><<<R, S_NT, L_TOTAL, s>>>(a);
    }
}
