// K14 for a MultiDiscrete head: the sub-heads' Categorical samples of ACTLayer.forward's multi-discrete branch
// (reference act.py:44-60: per sub-head FixedCategorical.sample / log_probs, then cat) in one launch, with the
// arithmetic of K14's categorical_sample_kernel (csrc/mappo_loss.hip).  The logits of all sub-heads are one
// [rows, sum n_k] matrix; sub-head k samples with its own noise tensor [rows, n_k], which the caller draws per sub-head
// in head order -- exactly the Exponential(1) draws of the framework's per-head torch.multinomial(p, 1) calls -- so
// actions and random stream are those of the framework path.  Log-probs stay per sub-head (not summed).
// One thread per row; at most MAPPO_MULTI_SAMPLE_MAX_HEADS sub-heads, sum n_k <= 64.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mappo_hip.h"
#include "../csrc/mappo_internal.h"

#pragma clang fp contract(off)

namespace {

struct MultiSampleArgs {
    const float* noise[MAPPO_MULTI_SAMPLE_MAX_HEADS];
    int size[MAPPO_MULTI_SAMPLE_MAX_HEADS];
    int heads, width;
};

__global__ void __launch_bounds__(256) multi_categorical_sample_kernel(const float* logits, MultiSampleArgs m,
                                                                       long long* actions, float* logp, long long rows) {
    const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
    if (r >= rows) return;
    const float* lg = logits + r * m.width;
    for (int h = 0; h < m.heads; ++h) {
        const int na = m.size[h];
        const float* q = m.noise[h] + r * na;
        float mx = -INFINITY;
        for (int i = 0; i < na; ++i) mx = fmaxf(mx, lg[i]);
        float se = 0.f;
        for (int i = 0; i < na; ++i) se += expf(lg[i] - mx);
        const float lse = mx + logf(se);
        int best = 0;
        float best_v = -1.f, best_l = 0.f;
        for (int i = 0; i < na; ++i) {
            const float l = lg[i] - lse;            // normalised logit = log p_i
            const float v = expf(l) / q[i];         // p_i / q_i (first maximum wins, like argmax)
            if (v > best_v) {
                best_v = v;
                best = i;
                best_l = l;
            }
        }
        actions[r * m.heads + h] = best;
        logp[r * m.heads + h] = best_l;
        lg += na;
    }
}

}  // namespace

extern "C" int mappo_multi_categorical_sample(const float* logits, const float* const* noise, const int* head_sizes,
                                              int num_heads, int64_t* actions, float* log_probs, int64_t rows,
                                              mappo_stream_t stream_) {
    if (!logits || !noise || !head_sizes || !actions || !log_probs) return MAPPO_E_NULL;
    if (rows <= 0 || num_heads <= 0 || num_heads > MAPPO_MULTI_SAMPLE_MAX_HEADS) return MAPPO_E_SHAPE;
    MultiSampleArgs m;
    m.heads = num_heads;
    m.width = 0;
    for (int h = 0; h < MAPPO_MULTI_SAMPLE_MAX_HEADS; ++h) {
        m.noise[h] = nullptr;
        m.size[h] = 0;
    }
    for (int h = 0; h < num_heads; ++h) {
        if (!noise[h]) return MAPPO_E_NULL;
        if (head_sizes[h] <= 0) return MAPPO_E_SHAPE;
        m.noise[h] = noise[h];
        m.size[h] = head_sizes[h];
        m.width += head_sizes[h];
    }
    if (m.width > 64) return MAPPO_E_SHAPE;
    hipLaunchKernelGGL(multi_categorical_sample_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0,
                       static_cast<hipStream_t>(stream_), logits, m, reinterpret_cast<long long*>(actions), log_probs,
                       (long long)rows);
    return (int)hipGetLastError();
}
