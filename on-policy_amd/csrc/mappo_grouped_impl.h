// K19: G small networks of one architecture, each on its own column slice of one joint observation row, evaluated -- and,
// for actors, sampled -- in ONE launch (included by mappo_mlp.hip after mappo_mlp_impl.h, whose layer tail it shares).
//
// A network is the reference's MLPBase at hidden size 64 plus one output Linear (onpolicy/algorithms/utils/mlp.py:33-58,
// distributions.py:55-68, r_actor_critic.py:147-175): [LayerNorm] -> (Linear -> Tanh | ReLU -> LayerNorm) x (1 + layer_N)
// -> Linear(64, out <= 32).  The separated runner's step has one actor and one critic per agent: up to 128 of them here.
//
// Grid: (row tiles of 32, networks).  A workgroup of four waves reads its descriptor from the device table with uniform
// (scalar) loads and owns 32 rows of one network.
//
//   First layer.  The source is a column view [rows, din] of a wider matrix -- any offset, any width up to kMaxDin, any row
//   stride -- so nothing about it is 16-byte aligned: both operands are streamed in chunks of kKC columns with 4-byte loads,
//   lane = column (a wave reads 256 consecutive bytes of one row), through registers into one LDS tile [32 + 64][kKC] of
//   odd row stride.  The next chunk's loads are issued before the current chunk's products, so the memory latency of a
//   chunk hides behind the 16 matrix instructions each wave issues on it.  The products are transposed, as in K9:
//   D[feature][row] = W1[feature][k] x[row][k], a wave's two accumulator tiles cover all 64 features of the 32 rows, and
//   the four waves split every chunk's columns (wave w: columns 8 w .. 8 w + 7 and 32 + 8 w .. 32 + 8 w + 7, which keeps
//   the two half-waves of an LDS read 32 banks apart).  Three waves then hand their partial tiles to wave 0 through LDS.
//
//   Input LayerNorm, in the SAME pass: a separate statistics pass would read a centralised critic's 9,139-float row twice,
//   the second time from L2 and before any product can start.  Instead every row is shifted by its first element p (in
//   registers, on its way to LDS: sums of x - p do not cancel for rows far from zero), the threads that carry a row's
//   columns to LDS accumulate sum (x - p) and sum (x - p)^2, the threads that carry a feature's weights multiply them by
//   gamma on the way and accumulate s_f = sum_k W gamma and t_f = sum_k W beta, and the first layer's pre-activation is
//   rstd (acc - (mean - p) s_f) + t_f + b.  Wave sums are taken once, after the last chunk.
//
//   Hidden layers and head: wave 0 alone (32 rows are one matrix-instruction tile, the launch is latency-sized and the
//   other waves stage the NEXT layer's 64 x 64 weights into the LDS region that is free meanwhile).  With the transposed
//   product a lane holds 32 of its row's 64 features and its partner half-wave the rest: LayerNorm statistics are an
//   in-lane sum and one exchange (mlp::layer_tail, K9's), and the registers are the next product's B operand as they are.
//   The head is one 32-wide tile; its outputs go to an LDS tile [32 rows][33].
//
//   Sampling: rows of an actor run K14's per-row body (mappo::sample_head, the function categorical_sample_kernel calls)
//   on that tile while it is on chip: same arithmetic, same bits.
//
// Plain float32 products on v_mfma_f32_32x32x2_f32 (the six-term bf16 form of K9 halves matrix time on 10^5 rows; here the
// matrix pipe is idle most of the launch).  No scratch, no atomics.  Rows past the last are clamped for loads and masked
// for stores; every barrier is reached by every thread.
#ifndef MAPPO_GROUPED_IMPL_H
#define MAPPO_GROUPED_IMPL_H

namespace grp {

constexpr int kKC = 64;                 // first-layer columns per chunk = lanes of a wave
constexpr int kS = kKC + 1;             // LDS row stride (floats) of every staged tile: odd, so a column walks the banks
constexpr int kTile = (32 + 64) * kS;   // floats: x chunk [32 rows][kKC] | W1 chunk [64 features][kKC]
constexpr int kThreads = 256;
constexpr int kMaxDin = MAPPO_GROUPED_MAX_DIN;

// feature of accumulator slot s = 16 t + v of a lane in half-wave h (prim::mfma32's D layout, tiles t = 0, 1)
__device__ __forceinline__ constexpr int feature_of(int s) { return 32 * (s >> 4) + (s & 3) + 8 * ((s & 15) >> 2); }

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) v += __shfl_xor(v, m);
    return v;
}

// dst [rows][kS] <- src [valid rows][64] (row-major, contiguous), zero rows behind; by the threads tid0 .. of `n` threads
__device__ __forceinline__ void stage_rows64(float* dst, const float* src, int rows, int valid, int t, int n) {
    for (int i = t; i < rows * 64; i += n) {
        const int r = i >> 6, k = i & 63;
        dst[r * kS + k] = r < valid ? src[r * 64 + k] : 0.f;
    }
}

// acc[t] = sum over the 64 features of W[32 t + c][feature] * (this row's feature), W staged [.][kS]
template <int TILES>
__device__ __forceinline__ void dense64(const float* w, int c, int h, const float* reg, f32x16* acc) {
#pragma unroll
    for (int t = 0; t < TILES; ++t)
#pragma unroll
        for (int v = 0; v < 16; ++v) acc[t][v] = 0.f;
#pragma unroll
    for (int s = 0; s < 32; ++s) {
        const int f = feature_of(s) + 4 * h;
#pragma unroll
        for (int t = 0; t < TILES; ++t) acc[t] = prim::mfma32(w[(32 * t + c) * kS + f], reg[s], acc[t]);
    }
}

__device__ __forceinline__ void tail(int act, const f32x16* acc, const float* vec, int h, float eps, float* hreg, int lane) {
    float mean, rstd;
    if (act == 1) mlp::layer_tail<false, 1>(acc, vec, h, eps, hreg, nullptr, lane, mean, rstd);
    else mlp::layer_tail<false, 2>(acc, vec, h, eps, hreg, nullptr, lane, mean, rstd);
}

// The shared arrays of a workgroup's trunk (declared by the kernel: the K19 kernels differ in what else they keep in LDS)
struct Lds {
    float* r1;                                      // [kTile] first layer: the chunk tile; then partial tiles, weights, logits
    float* r2;                                      // [64 * kS] the first hidden layer's weights; then head weights or logits
    float* vecs;                                    // [3 * 192], 16-byte aligned; per layer: bias | LayerNorm weight | bias
    float *head_b, *s_f, *t_f, *row_dm, *row_rstd;  // [32], [64], [64], [32], [32]
};
// ... and a thread's place in its workgroup's tile
struct Place {
    int tid, lane, wave, c, h, out;                 // (wave: uniform; c, h: the row and half-wave of a lane; out = d->out)
    long long row0;
};
__device__ __forceinline__ Place place_of(const mappo_grouped_net_t* d) {
    const int tid = threadIdx.x, lane = tid & 63;
    return Place{tid, lane, prim::uniform(tid >> 6), lane & 31, lane >> 5, d->out, (long long)blockIdx.x * 32};
}

// The trunk of network d on rows row0 .. row0 + 31: -> wave 0's hreg = the last block's LayerNorm output, 32 of its row's 64
// features per lane (feature_of).  HEAD: the output Linear's weights are staged on the way ([32][kS] at head_w, the other
// of r1 / r2 is `logits`); without it r1 and r2 are both free afterwards.  `early` runs on waves 1 .. 3 while wave 0 is in
// the first hidden layer (after their share of the staging).  Ends behind a barrier.
template <bool HEAD, class Early>
__device__ __forceinline__ void trunk(const mappo_grouped_net_t* d, long long rows, const Lds& lds, const Place& at, float* hreg,
                                      f32x16* acc, float*& head_w, float*& logits, Early early) {
    float* r1 = lds.r1;
    float* r2 = lds.r2;
    float* vecs = lds.vecs;
    float *head_b = lds.head_b, *s_f = lds.s_f, *t_f = lds.t_f, *row_dm = lds.row_dm, *row_rstd = lds.row_rstd;
    const int tid = at.tid, lane = at.lane, wave = at.wave, c = at.c, h = at.h, out = at.out;
    const long long row0 = at.row0;
    const int din = d->din, L = d->n_layers, act = d->act;
    const float eps = d->ln_eps;
    const float* w1 = d->w1;
    const float* in_g = d->in_g;
    const float* in_b = d->in_b;
    const bool in_ln = in_g != nullptr;
    float* xs = r1;
    float* ws = r1 + 32 * kS;
    for (int i = tid; i < L * 192; i += kThreads) {
        const int l = i / 192, j = i - 192 * l, part = j >> 6;
        const float* p = part == 0 ? d->bias[l] : part == 1 ? d->ln_g[l] : d->ln_b[l];
        vecs[i] = p[j & 63];
    }
    if (tid < 32) head_b[tid] = tid < out ? d->bh[tid] : 0.f;
    stage_rows64(r2, d->w2[0], 64, 64, tid, kThreads);

    // ---- first layer: this thread carries rows 4 i + wave (i < 8) and features 4 i + wave (i < 16) at column k0 + lane
    const float* xrow[8];
    float pivot[8], sum[8], sq[8], sacc[16], tacc[16];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        long long r = row0 + 4 * i + wave;
        r = r < rows ? r : rows - 1;
        xrow[i] = d->src + r * (long long)d->ld + d->col;
        pivot[i] = in_ln ? xrow[i][0] : 0.f;
        sum[i] = sq[i] = 0.f;
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) sacc[i] = tacc[i] = 0.f;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int v = 0; v < 16; ++v) acc[t][v] = 0.f;

    float xr[8], wr[16], gr = 1.f, br = 0.f;
    auto load_chunk = [&](int k0) {
        const int k = k0 + lane;
        const bool ok = k < din;
#pragma unroll
        for (int i = 0; i < 8; ++i) xr[i] = ok ? xrow[i][k] : 0.f;
#pragma unroll
        for (int i = 0; i < 16; ++i) wr[i] = ok ? w1[(long long)(4 * i + wave) * din + k] : 0.f;
        if (in_ln) {
            gr = ok ? in_g[k] : 0.f;
            br = ok ? in_b[k] : 0.f;
        }
    };
    load_chunk(0);
    for (int k0 = 0; k0 < din; k0 += kKC) {
        const bool ok = k0 + lane < din;
        __syncthreads();                            // the previous chunk's products have read the tile
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const float dx = ok ? xr[i] - pivot[i] : 0.f;
            xs[(4 * i + wave) * kS + lane] = dx;
            sum[i] += dx;
            sq[i] += dx * dx;
        }
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            float w = wr[i];
            if (in_ln) {
                tacc[i] += w * br;
                w *= gr;
                sacc[i] += w;
            }
            ws[(4 * i + wave) * kS + lane] = w;
        }
        __syncthreads();
        if (k0 + kKC < din) load_chunk(k0 + kKC);   // in flight under this chunk's products
#pragma unroll
        for (int kk = 0; kk < 8; ++kk) {
            const int k = 32 * h + 8 * wave + kk;
            const float b = xs[c * kS + k];
            acc[0] = prim::mfma32(ws[c * kS + k], b, acc[0]);
            acc[1] = prim::mfma32(ws[(32 + c) * kS + k], b, acc[1]);
        }
    }
    __syncthreads();                                // the tile is free: partial accumulators and statistics
    if (wave != 0) {
#pragma unroll
        for (int s = 0; s < 32; ++s) r1[((wave - 1) * 32 + s) * 64 + lane] = acc[s >> 4][s & 15];
    }
    if (in_ln) {
        const float inv = 1.f / (float)din;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const float m = wave_sum(sum[i]) * inv;                 // mean - pivot
            const float var = fmaxf(wave_sum(sq[i]) * inv - m * m, 0.f);
            if (lane == 0) {
                row_dm[4 * i + wave] = m;
                row_rstd[4 * i + wave] = 1.f / sqrtf(var + eps);
            }
        }
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const float s = wave_sum(sacc[i]), t = wave_sum(tacc[i]);
            if (lane == 0) {
                s_f[4 * i + wave] = s;
                t_f[4 * i + wave] = t;
            }
        }
    }
    __syncthreads();
    if (wave == 0) {
#pragma unroll
        for (int s = 0; s < 32; ++s)
            acc[s >> 4][s & 15] += r1[s * 64 + lane] + r1[(32 + s) * 64 + lane] + r1[(64 + s) * 64 + lane];
        if (in_ln) {
            const float dm = row_dm[c], rstd = row_rstd[c];
#pragma unroll
            for (int s = 0; s < 32; ++s) {
                const int f = feature_of(s) + 4 * h;
                acc[s >> 4][s & 15] = rstd * (acc[s >> 4][s & 15] - dm * s_f[f]) + t_f[f];
            }
        }
        tail(act, acc, vecs, h, eps, hreg, lane);
    }
    __syncthreads();                                // r1 is free

    // ---- hidden layers and head on wave 0; waves 1 .. 3 stage the weights of the step after
    if (wave != 0) {
        if (L == 3) stage_rows64(r1, d->w2[1], 64, 64, tid - 64, kThreads - 64);
        else if (HEAD) stage_rows64(r1, d->wh, 32, out, tid - 64, kThreads - 64);
        early();
    } else {
        dense64<2>(r2, c, h, hreg, acc);
        tail(act, acc, vecs + 192, h, eps, hreg, lane);
    }
    __syncthreads();
    head_w = r1;
    logits = r2;
    if (L == 3) {
        if (wave != 0) {
            if (HEAD) stage_rows64(r2, d->wh, 32, out, tid - 64, kThreads - 64);
        } else {
            dense64<2>(r1, c, h, hreg, acc);
            tail(act, acc, vecs + 384, h, eps, hreg, lane);
        }
        __syncthreads();
        head_w = r2;
        logits = r1;
    }
}

// The head on wave 0's hreg (weights [32][kS] at head_w) -> the tile logits [32 rows][33]; then y, and an actor's sampling
__device__ __forceinline__ void head_and_sample(const mappo_grouped_net_t* d, long long rows, const Place& at, const float* head_w,
                                                float* logits, const float* head_b, const float* hreg, f32x16* acc) {
    const int tid = at.tid, wave = at.wave, c = at.c, h = at.h, out = at.out;
    const long long row0 = at.row0;
    if (wave == 0) {
        dense64<1>(head_w, c, h, hreg, acc);        // D[output (v & 3) + 8 (v >> 2) + 4 h][row c]
#pragma unroll
        for (int v = 0; v < 16; ++v) {
            const int o = (v & 3) + 8 * (v >> 2) + 4 * h;
            logits[c * 33 + o] = acc[0][v] + head_b[o];
        }
    }
    __syncthreads();
    const long long left = rows - row0;             // > 0
    const int valid = left < 32 ? (int)left : 32;
    if (d->y) {
        for (int i = tid; i < valid * out; i += kThreads) {
            const int r = i / out;
            d->y[row0 * out + i] = logits[r * 33 + (i - r * out)];
        }
    }
    if (d->noise && tid < valid) {
        const long long r = row0 + tid;
        mappo::sample_head(logits + tid * 33, nullptr, d->noise + r * out, out,
                           reinterpret_cast<long long*>(d->actions) + r, d->logp + r);
    }
}

__global__ void __launch_bounds__(kThreads) grouped_nets_kernel(const mappo_grouped_net_t* table, long long rows) {
    __shared__ float r1[kTile];
    __shared__ float r2[64 * kS];
    __shared__ __attribute__((aligned(16))) float vecs[3 * 192];
    __shared__ float head_b[32], s_f[64], t_f[64], row_dm[32], row_rstd[32];

    const mappo_grouped_net_t* d = table + blockIdx.y;      // uniform: the descriptor is read with scalar loads
    const Lds lds = {r1, r2, vecs, head_b, s_f, t_f, row_dm, row_rstd};
    const Place at = place_of(d);
    float hreg[32];
    f32x16 acc[2];
    float *head_w, *logits;
    trunk<true>(d, rows, lds, at, hreg, acc, head_w, logits, [] {});
    head_and_sample(d, rows, at, head_w, logits, head_b, hreg, acc);
}

// ---- K19 recurrent: trunk -> GRU cell (recurrent_N = 1, 64 -> 64) -> LayerNorm -> head (-> sampling), per network, one launch
//
// The cell's six 64 x 64 products are 384 matrix instructions on 32 rows, as many again as a three-layer trunk.  They are
// laid out so that wave 0 -- the trunk's only worker after the first layer -- gets 96 of them:
//
//   hidden side   W_hh hm (hm = h_in * mask) needs nothing of the trunk.  Waves 1 and 2 take it, one per half of the 64
//                 features: three accumulator tiles each (r | z | n of their 32 features, all 32 rows; the transposed
//                 product of the trunk, D[feature][row]), 96 instructions, issued while wave 0 runs the trunk's first
//                 hidden layer.  The tiles then wait in (accumulator) registers.
//   input side    W_ih x starts behind the trunk's last tail: wave 0 puts x into an LDS tile, then waves 0 and 3 take a
//                 half of the features each (96 instructions) and hand their three tiles over through LDS, in register
//                 order: slot (gate, v) of lane l at [(gate, v)][l], so neither side's accesses conflict.
//   gates         where the hidden side waits: a lane of waves 1 / 2 holds r, z, n of 16 features of one row, reads hm
//                 from the tile the product read, and writes h' into the tile x came from.
//   out           waves 1 .. 3 copy that tile to h_out in whole rows (256-byte runs) while wave 0 reads it back in the
//                 trunk's register layout, normalises it (an in-lane sum and one exchange per moment, like layer_tail)
//                 and runs the head and the sampling as above.
//
// Both weight matrices are staged in LDS [192][kS] by all four waves before the first layer (B operands k = 32 h + s: the
// two half-waves of a read are 32 banks apart), W_ih too: its A operands are read 32 times per workgroup, and staging it
// later, from the one idle wave, would take that wave longer than the trunk's hidden layers last.  With the trunk's tiles
// that is 159 KB of the CU's 160: dynamic LDS, granted as for K12, one workgroup per CU -- what a latency-sized launch wants.
// The head's weights are staged behind the trunk (r2), the input side's tiles and then the logits go to r1.
constexpr int kRnnW = 192 * kS;                         // one staged GRU weight matrix
constexpr int kRnnVec = 6 * 64;                         // b_ir + b_hr | b_iz + b_hz | b_in | b_hn | LayerNorm weight | bias
constexpr int kRnnLds = 2 * kRnnW + 2 * 32 * kS + kRnnVec;      // floats: W_hh | W_ih | hm tile | x, then h' tile | vectors
static_assert(6 * 16 * 64 <= kTile, "the input side's six tiles pass through r1");

__global__ void __launch_bounds__(kThreads) grouped_rnn_nets_kernel(const mappo_grouped_rnn_net_t* table, long long rows) {
    __shared__ float r1[kTile];
    __shared__ float r2[64 * kS];
    __shared__ __attribute__((aligned(16))) float vecs[3 * 192];
    __shared__ float head_b[32], s_f[64], t_f[64], row_dm[32], row_rstd[32];
    float* whh = prim::lds();
    float* wih = whh + kRnnW;
    float* hmt = wih + kRnnW;                       // [32 rows][kS]
    float* xt = hmt + 32 * kS;                      // [32 rows][kS]
    float* gvec = xt + 32 * kS;

    const mappo_grouped_rnn_net_t* e = table + blockIdx.y;      // uniform, as above
    const mappo_grouped_net_t* d = &e->net;
    const Place at = place_of(d);
    const int tid = at.tid, lane = at.lane, wave = at.wave, c = at.c, h = at.h;
    const long long row0 = at.row0;
    const long long left = rows - row0;             // > 0
    const int valid = left < 32 ? (int)left : 32;

    stage_rows64(whh, e->w_hh, 192, 192, tid, kThreads);
    stage_rows64(wih, e->w_ih, 192, 192, tid, kThreads);
    for (int i = tid; i < 32 * 64; i += kThreads) {
        const int r = i >> 6, k = i & 63;
        hmt[r * kS + k] = r < valid ? e->h_in[(row0 + r) * 64 + k] * e->mask[row0 + r] : 0.f;
    }
    for (int i = tid; i < kRnnVec; i += kThreads) {
        const int part = i >> 6, f = i & 63;
        gvec[i] = part < 2 ? e->b_ih[64 * part + f] + e->b_hh[64 * part + f]
                           : part == 2 ? e->b_ih[128 + f] : part == 3 ? e->b_hh[128 + f] : part == 4 ? e->rnn_g[f] : e->rnn_b[f];
    }

    f32x16 gh[3];                                   // waves 1, 2: W_hh hm of gate g, features 32 (wave - 1) + ..., all rows
#pragma unroll
    for (int g = 0; g < 3; ++g)
#pragma unroll
        for (int v = 0; v < 16; ++v) gh[g][v] = 0.f;
    const Lds lds = {r1, r2, vecs, head_b, s_f, t_f, row_dm, row_rstd};
    float hreg[32];
    f32x16 acc[3];
    float *unused_w, *unused_l;
    trunk<false>(d, rows, lds, at, hreg, acc, unused_w, unused_l, [&] {
        if (wave != 3) {
            const float* w = whh + (32 * (wave - 1) + c) * kS + 32 * h;
            const float* b = hmt + c * kS + 32 * h;
#pragma unroll
            for (int s = 0; s < 32; ++s) {
                const float bv = b[s];
#pragma unroll
                for (int g = 0; g < 3; ++g) gh[g] = prim::mfma32(w[64 * g * kS + s], bv, gh[g]);
            }
        }
    });

    // ---- x into its tile; the head's weights behind the trunk
    if (wave == 0) {
#pragma unroll
        for (int s = 0; s < 32; ++s) xt[c * kS + feature_of(s) + 4 * h] = hreg[s];
    } else {
        stage_rows64(r2, d->wh, 32, at.out, tid - 64, kThreads - 64);
    }
    __syncthreads();
    // ---- input side: wave 0 features 0 .. 31, wave 3 features 32 .. 63
    if (wave == 0 || wave == 3) {
        const int half = wave == 3;
        const float* w = wih + (32 * half + c) * kS + 32 * h;
        const float* b = xt + c * kS + 32 * h;
#pragma unroll
        for (int g = 0; g < 3; ++g)
#pragma unroll
            for (int v = 0; v < 16; ++v) acc[g][v] = 0.f;
#pragma unroll
        for (int s = 0; s < 32; ++s) {
            const float bv = b[s];
#pragma unroll
            for (int g = 0; g < 3; ++g) acc[g] = prim::mfma32(w[64 * g * kS + s], bv, acc[g]);
        }
#pragma unroll
        for (int g = 0; g < 3; ++g)
#pragma unroll
            for (int v = 0; v < 16; ++v) r1[((3 * half + g) * 16 + v) * 64 + lane] = acc[g][v];
    }
    __syncthreads();
    // ---- gates on waves 1, 2: slot v is feature 32 half + (v & 3) + 8 (v >> 2) + 4 h of row c
    if (wave == 1 || wave == 2) {
        const int half = wave - 1;
#pragma unroll
        for (int v = 0; v < 16; ++v) {
            const int f = 32 * half + (v & 3) + 8 * (v >> 2) + 4 * h;
            const float* gi = r1 + (3 * half * 16 + v) * 64 + lane;
            const float hm = hmt[c * kS + f];
            const float r = gru::sigmoid_fast(gi[0] + gh[0][v] + gvec[f]);
            const float z = gru::sigmoid_fast(gi[16 * 64] + gh[1][v] + gvec[64 + f]);
            const float n = mlp::fast_tanh(gi[32 * 64] + gvec[128 + f] + r * (gh[2][v] + gvec[192 + f]));
            xt[c * kS + f] = (1.f - z) * n + z * hm;
        }
    }
    __syncthreads();
    // ---- h' out (waves 1 .. 3, whole rows); LayerNorm of it on wave 0, in the trunk's register layout
    if (wave != 0) {
        for (int i = tid - 64; i < valid * 64; i += kThreads - 64) e->h_out[row0 * 64 + i] = xt[(i >> 6) * kS + (i & 63)];
    } else {
        float sum = 0.f, var = 0.f;
#pragma unroll
        for (int s = 0; s < 32; ++s) {
            hreg[s] = xt[c * kS + feature_of(s) + 4 * h];
            sum += hreg[s];
        }
        sum += prim::xhalf(sum);
        const float mean = sum * (1.f / 64.f);
#pragma unroll
        for (int s = 0; s < 32; ++s) {
            hreg[s] -= mean;
            var += hreg[s] * hreg[s];
        }
        var += prim::xhalf(var);
        const float rstd = prim::rsq_fast(var * (1.f / 64.f) + d->ln_eps);
#pragma unroll
        for (int s = 0; s < 32; ++s) {
            const int f = feature_of(s) + 4 * h;
            hreg[s] = hreg[s] * rstd * gvec[256 + f] + gvec[320 + f];
        }
    }
    head_and_sample(d, rows, at, r2, r1, head_b, hreg, acc);
}

inline bool ok4(const void* p) { return mappo::aligned_to(p, 4); }

// MAPPO_E_* of one descriptor, 0 when the kernel takes it
inline int check(const mappo_grouped_net_t& n) {
    if (!n.src || !n.w1 || !n.wh || !n.bh || (!n.in_g) != (!n.in_b)) return MAPPO_E_NULL;
    if (n.n_layers < 2 || n.n_layers > MAPPO_MLP_MAX_LAYERS) return MAPPO_E_SHAPE;
    for (int l = 0; l < n.n_layers; ++l)
        if (!n.bias[l] || !n.ln_g[l] || !n.ln_b[l] || (l > 0 && !n.w2[l - 1])) return MAPPO_E_NULL;
    const bool actor = n.noise || n.actions || n.logp;
    if (actor ? (!n.noise || !n.actions || !n.logp) : !n.y) return MAPPO_E_NULL;
    if (n.hidden != 64 || n.out < 1 || n.out > MAPPO_GROUPED_MAX_OUT || n.din < 1 || n.din > kMaxDin) return MAPPO_E_SHAPE;
    if (n.col < 0 || n.ld < (int64_t)n.col + n.din || n.ld > INT32_MAX) return MAPPO_E_SHAPE;
    if (n.act != 1 && n.act != 2) return MAPPO_E_FLAGS;
    if (!(n.ln_eps > 0.f)) return MAPPO_E_SHAPE;
    const void* ptrs[] = {n.src, n.in_g, n.in_b, n.w1, n.bias[0], n.bias[1], n.bias[2], n.ln_g[0], n.ln_g[1], n.ln_g[2],
                          n.ln_b[0], n.ln_b[1], n.ln_b[2], n.w2[0], n.w2[1], n.wh, n.bh, n.y, n.noise, n.logp};
    for (const void* p : ptrs)
        if (!ok4(p)) return MAPPO_E_ALIGN;
    if (!mappo::aligned_to(n.actions, 8)) return MAPPO_E_ALIGN;
    return 0;
}

inline int prepare(const mappo_grouped_net_t* nets, int G, void* table) {
    if (!nets || !table) return MAPPO_E_NULL;
    if (G < 1 || G > MAPPO_GROUPED_MAX_NETS) return MAPPO_E_SHAPE;
    if (!mappo::aligned_to(table, 8)) return MAPPO_E_ALIGN;
    for (int g = 0; g < G; ++g) {
        const int e = check(nets[g]);
        if (e) return e;
    }
    return (int)hipMemcpy(table, nets, (size_t)G * sizeof(mappo_grouped_net_t), hipMemcpyHostToDevice);
}

inline int forward(const void* table, int G, long long rows, hipStream_t stream) {
    if (!table) return MAPPO_E_NULL;
    if (G < 1 || G > MAPPO_GROUPED_MAX_NETS || rows < 1 || rows > INT32_MAX) return MAPPO_E_SHAPE;
    hipLaunchKernelGGL(grouped_nets_kernel, dim3((unsigned)((rows + 31) / 32), (unsigned)G), dim3(kThreads), 0, stream,
                       static_cast<const mappo_grouped_net_t*>(table), rows);
    return (int)hipGetLastError();
}

// ... of one recurrent descriptor
inline int check(const mappo_grouped_rnn_net_t& n) {
    const int e = check(n.net);
    if (e) return e;
    const void* ptrs[] = {n.h_in, n.mask, n.h_out, n.w_ih, n.w_hh, n.b_ih, n.b_hh, n.rnn_g, n.rnn_b};
    for (const void* p : ptrs)
        if (!p) return MAPPO_E_NULL;
    if (n.h_out == n.h_in) return MAPPO_E_SHAPE;    // the state before the step stays what the caller put there
    for (const void* p : ptrs)
        if (!ok4(p)) return MAPPO_E_ALIGN;
    return 0;
}

inline int prepare(const mappo_grouped_rnn_net_t* nets, int G, void* table) {
    if (!nets || !table) return MAPPO_E_NULL;
    if (G < 1 || G > MAPPO_GROUPED_MAX_NETS) return MAPPO_E_SHAPE;
    if (!mappo::aligned_to(table, 8)) return MAPPO_E_ALIGN;
    for (int g = 0; g < G; ++g) {
        const int e = check(nets[g]);
        if (e) return e;
    }
    return (int)hipMemcpy(table, nets, (size_t)G * sizeof(mappo_grouped_rnn_net_t), hipMemcpyHostToDevice);
}

inline int forward_rnn(const void* table, int G, long long rows, hipStream_t stream) {
    if (!table) return MAPPO_E_NULL;
    if (G < 1 || G > MAPPO_GROUPED_MAX_NETS || rows < 1 || rows > INT32_MAX) return MAPPO_E_SHAPE;
    MAPPO_LAUNCH(grouped_rnn_nets_kernel, dim3((unsigned)((rows + 31) / 32), (unsigned)G), dim3(kThreads),
                 kRnnLds * sizeof(float), stream, static_cast<const mappo_grouped_rnn_net_t*>(table), rows);
    return MAPPO_LAUNCH_ERROR();
}

}  // namespace grp
#endif
