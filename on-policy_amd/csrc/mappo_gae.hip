// K1 -- GAE / discounted-return scan over the time-major rollout buffer, for gfx950.
//
// Replaces SharedReplayBuffer.compute_returns (reference onpolicy/utils/shared_buffer.py:179-262)
// and the advantage line of R_MAPPO.train (onpolicy/algorithms/r_mappo/r_mappo.py:179-182).
//
// The recurrence g_t = delta_t + (gamma*lambda*m_{t+1}) * g_{t+1} is serial along t and
// independent across the C = N*A columns, and the buffer is time-major ([T, C] rows), so
// lanes run along columns (coalesced rows) and every lane walks t = T-1 .. 0 with its
// carry in a register.  The arithmetic is the reference's float32 operation order with FMA
// contraction disabled => bit-identical to numpy.
//
// The scan is HBM-bound (16..24 B per (t, column) element, ~6 flops), and at the
// north-star size there are only C = 32768 columns = 512 wavefronts for 256 CUs, so
// bandwidth comes from memory-level parallelism per wave, not from occupancy.  The kernels:
//   * gae_dma_epi_kernel (variants 57, 54, 56: the automatic choice from 8192 columns up): a
//     workgroup owns a strip of W columns; producer waves stream [TC rows x W cols] tiles of
//     every input field straight into an LDS ring with 128-bit LDS-DMA loads, one walker wave
//     per 64 columns walks each tile backwards in time out of LDS, and the producers run the
//     epilogue (returns / advantages / moments) one tile behind the walker.
//   * gae_dma_kernel (variant 36, narrower buffers): the same ring; the walker stores its own
//     results.
//   * gae_scan_kernel (variant 70): time-parallel scan for narrow buffers, tolerance mode.
//   * gae_column_kernel (variant 99 and every number without a kernel of its own): one lane per
//     column with plain 4-byte loads; any C, any alignment, and the non-GAE modes.
//   * gae_mat_kernel (the multi-agent-transformer branches) and the advantage / moment kernels
//     (K5) behind their own entry points.
// The shapes that tuning tried and dropped (cooperative strips, a register-prefetch pipe, other
// ring shapes and depths, a 16-column scan) are no longer built; their A/B records remain under
// profiles/.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stdint.h>
#include <type_traits>

#include "mappo_hip.h"
#include "mappo_internal.h"

#pragma clang fp contract(off)
typedef float vf4 __attribute__((ext_vector_type(4)));

namespace {

struct GaeArgs {
    const float* rewards;
    float* value_preds;
    const float* next_value;
    const float* masks;
    const float* bad;
    float* returns;
    const float* denorm;
    float* adv;
    const float* active;
    double* partials;
    long long partial_rows;  // rows of `partials`; rows >= gridDim.x are zero-filled by block 0
    int opts;                // tuning bits: 1 = XCD-contiguous strip order, 2 = non-temporal DMA loads
    int T;
    long long C;
    float gamma;
    float gl;  // float32(gamma_f64 * lambda_f64), shared_buffer.py:239
};

// One backward step of the reference's GAE branches (shared_buffer.py:192-203 PTL,
// :236-240 / :255-258 no PTL).  dv1 = D(v_{t+1}) carried from the previous step.
template <bool PTL, bool DENORM>
__device__ __forceinline__ float gae_step(float r, float v0, float m1, float bad1, float sigma,
                                          float mu, float gamma, float gl, float& dv1, float& g,
                                          float& dv0_out) {
    float dv0 = v0;
    if (DENORM) {
        float s = v0 * sigma;  // valuenorm.py:75: x * sqrt(var) + mean, two roundings
        dv0 = s + mu;
    }
    float gv = gamma * dv1;
    float gvm = gv * m1;
    float rp = r + gvm;
    float delta = rp - dv0;
    float carry;
    if (PTL && DENORM) {
        float x = gl * g;  // shared_buffer.py:195: gamma*lambda*gae*mask
        carry = x * m1;
    } else {
        float x = gl * m1;  // shared_buffer.py:201,239,257: gamma*lambda*mask*gae
        carry = x * g;
    }
    g = delta + carry;
    if (PTL) g = g * bad1;
    float ret = g + dv0;
    dv1 = dv0;
    dv0_out = dv0;
    return ret;
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

// One row of the partials array: the wave's three moments, written by its lane 0.
__device__ __forceinline__ void write_partials(const GaeArgs& a, long long row, int lane, double s1, double s2,
                                               double cnt) {
    if (a.partials != nullptr) {
        s1 = wave_sum(s1);
        s2 = wave_sum(s2);
        cnt = wave_sum(cnt);
        if (lane == 0) {
            double* p = a.partials + row * 3;
            p[0] = s1;
            p[1] = s2;
            p[2] = cnt;
        }
    }
}

// D(v) = v * sigma + mu of the value normaliser (valuenorm.py:75); the identity without one.
__device__ __forceinline__ void load_denorm(const GaeArgs& a, bool denorm, float& sigma, float& mu) {
    sigma = 1.f;
    mu = 0.f;
    if (denorm) {
        sigma = a.denorm[0];
        mu = a.denorm[1];
    }
}


// Rows of the partials array that no workgroup owns are zeroed by workgroup 0, so that the
// fixed-size reduction needs no separate memset launch.
__device__ __forceinline__ void zero_unowned_partials(double* partials, long long rows, int per_block = 1) {
    if (partials != nullptr && blockIdx.x == 0) {
        for (long long r = (long long)gridDim.x * per_block + threadIdx.x; r < rows; r += blockDim.x) {
            partials[r * 3 + 0] = 0.0;
            partials[r * 3 + 1] = 0.0;
            partials[r * 3 + 2] = 0.0;
        }
    }
}

// ------------------------------------------------------------------ ring kernels ----
// A tile is TC consecutive time steps of one strip of W columns; in LDS it is [slot][TC][W] floats
// with slots r, v, m, [bad], [active].
//
// Walk one tile backwards in time out of LDS (one lane per column).  The walker wave is the serial
// part of the kernel (400 dependent steps), so its instruction stream is kept lean:
//   * the LDS operands of U consecutive steps are fetched in one batch before they are needed (they
//     do not depend on the recurrence), so one LDS round trip is exposed per U steps, not per step;
//   * no per-step branches: dead lanes leave before the loop (there is no barrier inside), the
//     moment accumulation uses selects, output pointers are decremented instead of recomputed.
template <int W, int TC, bool PTL, bool DENORM, bool ACT, bool ADV>
__device__ __forceinline__ void walk_tile_impl(const GaeArgs& a, const float* ldsf, int lane, long long col,
                                               bool live, int tbase, float sigma, float mu, float& g,
                                               float& dv1, double& s1, double& s2, double& cnt, int lds_col) {
    constexpr int TILE = TC * W;
    constexpr int U = TC % 8 == 0 ? 8 : (TC % 4 == 0 ? 4 : (TC % 2 == 0 ? 2 : 1));
    static_assert(TC % U == 0, "tile length vs walker batch");
    if (!live) return;
    // LDS column of this lane: its lane for strips up to one wave wide, or the caller's column for
    // strips shared by several walker waves
    const int lc = lds_col >= 0 ? lds_col : lane;
    const float* lr = ldsf + 0 * TILE + lc;
    const float* lv = ldsf + 1 * TILE + lc;
    const float* lm = ldsf + 2 * TILE + lc;
    const float* lb = ldsf + 3 * TILE + lc;
    const float* la = ldsf + (PTL ? 4 : 3) * TILE + lc;
    const int slo = tbase < 0 ? -tbase : 0;            // rows below t = 0 do not exist (last tile only)
    const float gamma = a.gamma, gl = a.gl;
    const long long C = a.C;
    float* pret = a.returns + (long long)(tbase + TC - 1) * C + col;
    float* padv = ADV ? a.adv + (long long)(tbase + TC - 1) * C + col : nullptr;
    for (int s0 = TC - 1; s0 >= slo; s0 -= U) {
        float r[U], v0[U], m1[U], b1[U], am[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int s = s0 - u;                      // always inside the tile (TC % U == 0)
            r[u] = lr[s * W];
            v0[u] = lv[s * W];
            m1[u] = lm[s * W];
            b1[u] = PTL ? lb[s * W] : 1.f;
            am[u] = ACT ? la[s * W] : 1.f;
        }
        const int nvalid = s0 - slo + 1 < U ? s0 - slo + 1 : U;
        if (nvalid == U) {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                float dv0;
                float ret = gae_step<PTL, DENORM>(r[u], v0[u], m1[u], b1[u], sigma, mu, gamma, gl, dv1, g, dv0);
                *pret = ret;
                pret -= C;
                if (ADV) {
                    float adv = ret - dv0;             // r_mappo.py:180 (from the rounded return)
                    *padv = adv;
                    padv -= C;
                    double d = (am[u] != 0.f) ? (double)adv : 0.0;
                    s1 += d;
                    s2 += d * d;
                    cnt += (am[u] != 0.f) ? 1.0 : 0.0;
                }
            }
        } else {
            for (int u = 0; u < nvalid; ++u) {
                float dv0;
                float ret = gae_step<PTL, DENORM>(r[u], v0[u], m1[u], b1[u], sigma, mu, gamma, gl, dv1, g, dv0);
                *pret = ret;
                pret -= C;
                if (ADV) {
                    float adv = ret - dv0;
                    *padv = adv;
                    padv -= C;
                    double d = (am[u] != 0.f) ? (double)adv : 0.0;
                    s1 += d;
                    s2 += d * d;
                    cnt += (am[u] != 0.f) ? 1.0 : 0.0;
                }
            }
        }
    }
}

template <int W, int TC, bool PTL, bool DENORM, bool ACT>
__device__ __forceinline__ void walk_tile(const GaeArgs& a, const float* ldsf, int lane, long long col,
                                          bool live, int tbase, float sigma, float mu, float& g,
                                          float& dv1, double& s1, double& s2, double& cnt, int lds_col = -1) {
    if (a.adv != nullptr)   // wave-uniform: the fused-epilogue and the plain loop are separate code
        walk_tile_impl<W, TC, PTL, DENORM, ACT, true>(a, ldsf, lane, col, live, tbase, sigma, mu, g, dv1, s1, s2,
                                                      cnt, lds_col);
    else
        walk_tile_impl<W, TC, PTL, DENORM, ACT, false>(a, ldsf, lane, col, live, tbase, sigma, mu, g, dv1, s1,
                                                       s2, cnt, lds_col);
}

// The walker's start: the bootstrap value goes into row T of value_preds, D() of it is the first
// step's dv1.
__device__ __forceinline__ float walker_prologue(const GaeArgs& a, bool live, long long col, bool denorm,
                                                 float sigma, float mu) {
    float dv1 = 0.f;
    if (live) {
        float nv = a.next_value[col];
        a.value_preds[(long long)a.T * a.C + col] = nv;  // shared_buffer.py:187,218
        dv1 = nv;
        if (denorm) {
            float s = nv * sigma;
            dv1 = s + mu;
        }
    }
    return dv1;
}

// ---- "dma" kernel: producers stream tiles straight into an LDS ring with LDS-DMA ---------
// (global_load_lds_dwordx4: global -> LDS without passing through VGPRs, gfx950).  One walker
// wave + NPROD producer waves per strip of W columns; the ring holds R tiles of TC steps.
// While the walker consumes tile k, tiles k+1 .. k+R-1 are in flight or landed.  The DMA
// loads are issued from inline asm, so the compiler neither counts nor drains them: the
// producers wait for exactly the oldest tile with a counted s_waitcnt vmcnt(N) and then meet
// the walker at one s_barrier per tile (DMA data is visible to other waves after the issuing
// wave's vmcnt wait + a barrier).
//
// One wave instruction moves 64 lanes x 16 B = 1 KiB: RPI = 256 / W consecutive tile rows of
// one field; LDS destination = wave-uniform base + lane * 16 (so a tile slot is [TC][W] floats,
// rows contiguous), global source address is per lane.
template <bool NT>
__device__ __forceinline__ void lds_dma_16B(const float* gsrc, unsigned lds_dst) {
    unsigned keep;
    if (NT)
        asm volatile(
            "s_mov_b32 %0, m0\n\t"
            "s_mov_b32 m0, %2\n\t"
            "s_nop 0\n\t"
            "global_load_lds_dwordx4 %1, off nt\n\t"
            "s_mov_b32 m0, %0"
            : "=&s"(keep)
            : "v"(gsrc), "s"(lds_dst)
            : "memory");
    else
        asm volatile(
            "s_mov_b32 %0, m0\n\t"
            "s_mov_b32 m0, %2\n\t"
            "s_nop 0\n\t"
            "global_load_lds_dwordx4 %1, off\n\t"
            "s_mov_b32 m0, %0"
            : "=&s"(keep)
            : "v"(gsrc), "s"(lds_dst)
            : "memory");
}

// Workgroup -> strip.  Workgroup b runs on XCD b % 8 (observed placement, used for speed only):
// with opts bit 0 the strips of one XCD are consecutive, so each XCD's L2 / fabric port streams
// contiguous 64 * W * 4-byte row segments instead of every 8th 256-byte piece.
__device__ __forceinline__ unsigned strip_of_block(const GaeArgs& a) {
    const unsigned b = blockIdx.x, nb = gridDim.x;
    if ((a.opts & 1) && (nb % 8u) == 0u) return (b % 8u) * (nb / 8u) + b / 8u;
    return b;
}

template <int N>
__device__ __forceinline__ void wait_vmcnt() {
    static_assert(N >= 0 && N < 64, "vmcnt is a 6-bit counter");
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// The producers' DMA issue path of both ring kernels.  Loads are branch-free: out-of-range rows /
// columns are CLAMPED to a valid address instead of predicated, so that every tile is the same
// straight-line sequence of LPT instructions per producer wave and the counted waits below hold.
template <int W, int TC, int NPROD, int NF, bool PTL>
struct TileDma {
    static constexpr int RPI = 256 / W;            // tile rows per wave instruction
    static constexpr int IPS = TC / RPI;           // instructions per slot (field) per tile
    static constexpr int LPT = NF * IPS / NPROD;   // instructions per producer wave per tile
    static constexpr int TILE_FLOATS = NF * TC * W;
    static_assert(W <= 256 && (W <= 64 || W % 64 == 0), "strip width");
    static_assert(TC % RPI == 0 && IPS % NPROD == 0, "row groups must split evenly over the producers");

    const float *fb0, *fb1, *fb2, *fb3, *fb4;      // field bases at this lane's (clamped) column
    long long C;
    unsigned lds_base;                             // LDS byte address of the ring
    int pw, r0;                                    // producer index; this lane's row (of RPI) inside one instruction
    bool nt;

    __device__ __forceinline__ TileDma(const GaeArgs& a, long long col0, const float* ring, int pw_, int lane)
        : C(a.C), lds_base((unsigned)(uintptr_t)ring), pw(pw_), nt((a.opts & 2) != 0) {
        const int row = lane / (W / 4);
        const int c4 = lane - row * (W / 4);       // this lane's 4-column group
        r0 = row;
        long long lc = col0 + c4 * 4;
        if (lc > C - 4) lc = C - 4;                // clamp instead of predicating
        fb0 = a.rewards + lc;
        fb1 = a.value_preds + lc;
        fb2 = a.masks + C + lc;                    // masks / bad_masks are read at row t+1
        fb3 = (PTL ? a.bad + C : a.active) + lc;
        fb4 = a.active + lc;
    }

    // tile with time base `tbase` -> ring slot `slot`; field index is compile-time, this wave
    // takes row groups pw, pw + NPROD, ... of every field
    __device__ __forceinline__ void issue_tile(int tbase, int slot) const {
        const unsigned slot_addr = lds_base + (unsigned)slot * (TILE_FLOATS * 4);
#pragma unroll
        for (int s = 0; s < NF; ++s) {
            const float* fbs = s == 0 ? fb0 : s == 1 ? fb1 : s == 2 ? fb2 : (s == 3 && PTL) ? fb3 : fb4;
#pragma unroll
            for (int q = 0; q < IPS / NPROD; ++q) {
                const int rg = pw + q * NPROD;     // row group inside the tile
                int t = tbase + rg * RPI + r0;
                if (t < 0) t = 0;
                const float* src = fbs + (long long)t * C;
                const unsigned dst = slot_addr + (unsigned)((s * TC + rg * RPI) * W * 4);
                if (nt) lds_dma_16B<true>(src, dst);
                else lds_dma_16B<false>(src, dst);
            }
        }
    }
};

template <int W, int NPROD, int TC, int R, bool PTL, bool DENORM, bool ACT>
__global__ void __launch_bounds__((NPROD + (W + 63) / 64) * 64) gae_dma_kernel(GaeArgs a) {
    constexpr int NWALK = (W + 63) / 64;           // walker waves (64 columns each)
    constexpr int NF = 3 + (PTL ? 1 : 0) + (ACT ? 1 : 0);
    using Dma = TileDma<W, TC, NPROD, NF, PTL>;
    constexpr int LPT = Dma::LPT;
    constexpr int TILE_FLOATS = Dma::TILE_FLOATS;
    static_assert(R >= 2 && (R - 2) * LPT < 64, "ring depth vs the 6-bit vmcnt");
    static_assert(R * TILE_FLOATS * 4 <= 160 * 1024, "LDS ring");

    extern __shared__ vf4 lds4[];                  // [R][NF][TC][W / 4]
    float* ldsf = reinterpret_cast<float*>(lds4);
    const int T = a.T;
    const int nch = (T + TC - 1) / TC;
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    const long long col0 = (long long)strip_of_block(a) * W;
    zero_unowned_partials(a.partials, a.partial_rows, NWALK);

    if (wave < NWALK) {
        const int lane = threadIdx.x & 63;
        const int lds_col = NWALK > 1 ? wave * 64 + lane : -1;
        const long long col = col0 + (NWALK > 1 ? wave * 64 : 0) + lane;
        const bool live = (NWALK > 1 || lane < W) && col < a.C;
        float sigma, mu, g = 0.f;
        double s1 = 0.0, s2 = 0.0, cnt = 0.0;
        load_denorm(a, DENORM, sigma, mu);
        float dv1 = walker_prologue(a, live, col, DENORM, sigma, mu);
        __syncthreads();                                        // tile 0 landed
        int slot = 0;
        for (int k = 0; k < nch; ++k) {
            walk_tile<W, TC, PTL, DENORM, ACT>(a, ldsf + slot * TILE_FLOATS, lane, col, live,
                                               T - (k + 1) * TC, sigma, mu, g, dv1, s1, s2, cnt, lds_col);
            slot = slot + 1 == R ? 0 : slot + 1;
            __syncthreads();                                    // tile k+1 landed, tile k released
        }
        write_partials(a, (long long)blockIdx.x * NWALK + wave, lane, s1, s2, cnt);
    } else {
        const Dma dma(a, col0, ldsf, wave - NWALK, threadIdx.x & 63);
        // prologue: tiles 0 .. R-2 in flight, wait for tile 0
#pragma unroll
        for (int m = 0; m < R - 1; ++m) dma.issue_tile(T - (m + 1) * TC, m);
        wait_vmcnt<(R - 2) * LPT>();
        __syncthreads();
        int slot = R - 1;                     // ring slot of tile k + R - 1
        for (int k = 0; k < nch; ++k) {
            dma.issue_tile(T - (k + R) * TC, slot);   // the slot the walker released at the last barrier
            slot = slot + 1 == R ? 0 : slot + 1;
            wait_vmcnt<(R - 2) * LPT>();      // tile k+1 has landed; k+2 .. k+R-1 stay in flight
            __syncthreads();
        }
        wait_vmcnt<0>();
    }
}

// ---- "dma-epi" kernel: the DMA ring kernel with the epilogue moved off the walker ---------
// The walker wave is the serial critical path, so here it does nothing but the recurrence: it reads
// r, v, m[, bad] from the LDS tile and writes the return of every step into a small LDS output
// tile.  The producer waves -- idle between DMA issues -- run the whole epilogue one tile behind:
// they re-derive D(v) (same two roundings as the walker), form the advantage from the rounded
// return, store returns / advantages with 16-byte row-contiguous stores and accumulate the float64
// moments across all their lanes.  Timeline of barrier interval k (tile k is being walked):
//   producers: issue DMA of tile k+R-2 (into the slot of tile k-2) -> epilogue of tile k-1 ->
//              counted wait until tile k+1 has landed -> barrier.
// The ring therefore holds tiles k-1 .. k+R-2; the output tile is double buffered.
// LDS of one instance: the ring plus the two output tiles.  Every shape that is built holds its
// whole ring with all five input fields (static_assert in launch_dma_epi).
constexpr size_t epi_lds_bytes(int R, int NF, int TC, int W) {
    return ((size_t)R * NF + 2) * TC * W * sizeof(float);
}

template <int W, int NPROD, int TC, int R, bool PTL, bool DENORM, bool ACT>
__global__ void __launch_bounds__((NPROD + (W + 63) / 64) * 64) gae_dma_epi_kernel(GaeArgs a) {
    constexpr int NWALK = (W + 63) / 64;
    constexpr int NF = 3 + (PTL ? 1 : 0) + (ACT ? 1 : 0);
    using Dma = TileDma<W, TC, NPROD, NF, PTL>;
    constexpr int LPT = Dma::LPT;                  // DMA instructions per producer wave per tile
    constexpr int TILE = TC * W;                   // floats per field per tile
    constexpr int TILE_FLOATS = Dma::TILE_FLOATS;
    constexpr int V = W / 4;
    constexpr int GROUPS = TC * V;                 // float4 groups per tile
    constexpr int GPL = (GROUPS + NPROD * 64 - 1) / (NPROD * 64);   // groups per producer lane
    static_assert(R >= 3 && (R - 3) * LPT < 64, "ring depth vs the 6-bit vmcnt");
    static_assert(epi_lds_bytes(R, NF, TC, W) <= 160 * 1024, "LDS ring + output tiles");

    extern __shared__ vf4 lds4[];                  // [R][NF][TC][V] ring, then [2][TC][V] output tiles
    float* ldsf = reinterpret_cast<float*>(lds4);
    float* outf = ldsf + R * TILE_FLOATS;
    const int T = a.T;
    const int nch = (T + TC - 1) / TC;
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    const long long col0 = (long long)strip_of_block(a) * W;
    const long long C = a.C;
    zero_unowned_partials(a.partials, a.partial_rows, NPROD);

    float sigma, mu;
    load_denorm(a, DENORM, sigma, mu);

    if (wave < NWALK) {
        // ---------------------------------------------------------------- walker
        const int lane = threadIdx.x & 63;
        const int lc = NWALK > 1 ? wave * 64 + lane : lane;
        const long long col = col0 + lc;
        const bool live = lc < W && col < C;
        float dv1 = walker_prologue(a, live, col, DENORM, sigma, mu), g = 0.f;
        const float gamma = a.gamma, gl = a.gl;
        constexpr int U = TC % 8 == 0 ? 8 : (TC % 4 == 0 ? 4 : (TC % 2 == 0 ? 2 : 1));
        __syncthreads();                                        // tile 0 landed
        int slot = 0;
        for (int k = 0; k < nch; ++k) {
            if (live) {
                const float* base = ldsf + slot * TILE_FLOATS + lc;
                float* po = outf + (k & 1) * TILE + lc;
                for (int s0 = TC - 1; s0 >= 0; s0 -= U) {       // rows below t = 0 are computed but never stored
                    float r[U], v0[U], m1[U], b1[U];
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        const int sidx = (s0 - u) * W;
                        r[u] = base[0 * TILE + sidx];
                        v0[u] = base[1 * TILE + sidx];
                        m1[u] = base[2 * TILE + sidx];
                        b1[u] = PTL ? base[3 * TILE + sidx] : 1.f;
                    }
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        float dv0;
                        po[(s0 - u) * W] = gae_step<PTL, DENORM>(r[u], v0[u], m1[u], b1[u], sigma, mu, gamma, gl,
                                                                 dv1, g, dv0);
                    }
                }
            }
            slot = slot + 1 == R ? 0 : slot + 1;
            __syncthreads();                                    // tile k+1 landed; output tile k published
        }
    } else {
        // -------------------------------------------------------------- producers
        const int lane = threadIdx.x & 63;
        const int pw = wave - NWALK;
        const int ptid = pw * 64 + lane;                        // index among the producer lanes
        const Dma dma(a, col0, ldsf, pw, lane);
        const bool has_adv = a.adv != nullptr;
        double s1 = 0.0, s2 = 0.0, cnt = 0.0;

        // epilogue of tile m (walked during the previous interval): returns / advantages / moments
        auto epilogue = [&](int m) {
            const int tbase = T - (m + 1) * TC;
            const float* in = ldsf + (m % R) * TILE_FLOATS;
            const float* out = outf + (m & 1) * TILE;
#pragma unroll
            for (int q = 0; q < GPL; ++q) {
                const int i = ptid + q * NPROD * 64;
                const int row = i / V;
                const int cg = i - row * V;
                const int t = tbase + row;
                const long long col = col0 + cg * 4;
                if (i < GROUPS && t >= 0 && col < C) {
                    const vf4 ret = *reinterpret_cast<const vf4*>(out + row * W + cg * 4);
                    const long long o = (long long)t * C + col;
                    __builtin_nontemporal_store(ret, reinterpret_cast<vf4*>(a.returns + o));
                    if (has_adv) {
                        const vf4 v = *reinterpret_cast<const vf4*>(in + 1 * TILE + row * W + cg * 4);
                        vf4 am = vf4(1.f);
                        if (ACT) am = *reinterpret_cast<const vf4*>(in + (PTL ? 4 : 3) * TILE + row * W + cg * 4);
                        vf4 adv;
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            float dv0 = v[e];
                            if (DENORM) {
                                float sc = v[e] * sigma;   // valuenorm.py:75, same two roundings as the walker
                                dv0 = sc + mu;
                            }
                            adv[e] = ret[e] - dv0;          // r_mappo.py:180 (from the rounded return)
                            double d = (am[e] != 0.f) ? (double)adv[e] : 0.0;
                            s1 += d;
                            s2 += d * d;
                            cnt += (am[e] != 0.f) ? 1.0 : 0.0;
                        }
                        __builtin_nontemporal_store(adv, reinterpret_cast<vf4*>(a.adv + o));
                    }
                }
            }
        };

        // prologue: tiles 0 .. R-3 in flight, wait for tile 0
#pragma unroll
        for (int m = 0; m < R - 2; ++m) dma.issue_tile(T - (m + 1) * TC, m);
        wait_vmcnt<(R - 3) * LPT>();
        __syncthreads();
        int slot = R - 2;                     // ring slot of tile k + R - 2
        for (int k = 0; k < nch; ++k) {
            dma.issue_tile(T - (k + R - 1) * TC, slot);         // tile k+R-2 -> the slot tile k-2 has left
            slot = slot + 1 == R ? 0 : slot + 1;
            if (k >= 1) epilogue(k - 1);
            wait_vmcnt<(R - 3) * LPT>();                        // tile k+1 has landed
            __syncthreads();
        }
        epilogue(nch - 1);
        write_partials(a, (long long)blockIdx.x * NPROD + pw, lane, s1, s2, cnt);
        wait_vmcnt<0>();
    }
}

// ----------------------------------------------------------------- column kernel ----
// One lane per column, any C, all seven reference branches.
template <bool GAE, bool PTL, bool DENORM>
__global__ void __launch_bounds__(64) gae_column_kernel(GaeArgs a) {
    const long long C = a.C;
    const int T = a.T;
    const long long col = (long long)blockIdx.x * 64 + threadIdx.x;
    const bool live = col < C;
    const bool has_act = a.active != nullptr;
    const bool has_adv = a.adv != nullptr;

    float sigma, mu;
    load_denorm(a, DENORM, sigma, mu);
    const float gamma = a.gamma, gl = a.gl;
    double s1 = 0.0, s2 = 0.0, cnt = 0.0;

    if (live) {
        float nv = a.next_value[col];
        float g = 0.f, dv1 = 0.f, ret1 = nv;
        if (GAE) {
            a.value_preds[(long long)T * C + col] = nv;
            dv1 = nv;
            if (DENORM) {
                float s = nv * sigma;
                dv1 = s + mu;
            }
        } else {
            a.returns[(long long)T * C + col] = nv;  // shared_buffer.py:205,260
        }
        constexpr int U = 4;
        for (int thi = T - 1; thi >= 0; thi -= U) {
            float r[U], v0[U], m1[U], bad1[U], am[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                int t = thi - u;
                bool ok = t >= 0;
                long long o = (long long)(ok ? t : 0) * C + col;
                r[u] = a.rewards[o];
                v0[u] = a.value_preds[o];
                m1[u] = a.masks[o + C];
                bad1[u] = PTL ? a.bad[o + C] : 1.f;
                am[u] = has_act ? a.active[o] : 1.f;
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                int t = thi - u;
                if (t < 0) break;
                long long o = (long long)t * C + col;
                float ret, dv0;
                if (GAE) {
                    ret = gae_step<PTL, DENORM>(r[u], v0[u], m1[u], bad1[u], sigma, mu, gamma, gl,
                                                dv1, g, dv0);
                } else {
                    dv0 = v0[u];
                    if (DENORM) {
                        float s = v0[u] * sigma;
                        dv0 = s + mu;
                    }
                    float x = ret1 * gamma;  // shared_buffer.py:208,213,262
                    float y = x * m1[u];
                    float z = y + r[u];
                    if (PTL) {
                        float zb = z * bad1[u];
                        float ob = 1.f - bad1[u];
                        float w = ob * dv0;
                        ret = zb + w;
                    } else {
                        ret = z;
                    }
                    ret1 = ret;
                }
                a.returns[o] = ret;
                if (has_adv) {
                    float adv = ret - dv0;
                    a.adv[o] = adv;
                    if (am[u] != 0.f) {
                        double d = (double)adv;
                        s1 += d;
                        s2 += d * d;
                        cnt += 1.0;
                    }
                }
            }
        }
    }
    zero_unowned_partials(a.partials, a.partial_rows);
    write_partials(a, blockIdx.x, threadIdx.x, s1, s2, cnt);
}

// ------------------------------------------------------------------ time-parallel scan ----
// Narrow buffers (C = N * A of a few thousand columns: cfg2, SMAC, one rank's shard of a data-parallel job) do not
// have enough columns to hide a 200 .. 400-step serial walk: the ring kernels above sit on a ~40-60 us latency floor
// whatever the byte count.  The recurrence g_t = delta_t + c_t * g_{t+1} is an affine map in g, and affine maps
// compose: a segment [t0, t1) acts as g_{t0} = Q + P * g_{t1} with (P, Q) computable without knowing g_{t1}.
// A workgroup takes 32 columns x all T steps; T is cut into 16 segments, one per half-wave (8 waves x 2).  Every lane
//   1. loads ITS segment of ITS column into registers -- all loads of the tile are in flight at once, the memory
//      system sees the whole problem instead of one time step after the other;
//   2. folds the segment into (P, Q) walking backwards;
//   3. after one barrier composes the (P, Q) of the later segments (<= 15 fused multiply-adds) into its incoming g;
//   4. walks its segment again -- now with the true incoming g and the REFERENCE's operation order (gae_step) --
//      writing returns / advantages / moments.
// Only the 15 segment-boundary values carry the re-association error of step 3 (a few ulp); everything inside a segment
// is the bit-exact recurrence started from them.  Hence "tolerance mode": results agree with the reference to ~1e-6
// relative instead of bit for bit, which is what BASELINE.json's north star asks of returns / advantages.  Selected for
// 2048 <= C < 16384 (wide buffers keep the bit-exact ring kernels; MAPPO_GAE_EXACT forces them everywhere).
constexpr int kScanSegs = 16;
constexpr int kScanLmax = 26;      // steps per segment held in registers: T <= 416

// W columns per workgroup, 64 / W segments per wave.  Built for W = 32: 8 waves, 128-byte row pieces, C / 32 workgroups.
template <int W, bool PTL, bool DENORM, bool ACT>
__global__ void __launch_bounds__(W * kScanSegs) gae_scan_kernel(GaeArgs a) {
    constexpr int kScanCols = W;
    constexpr int NWAVES = W * kScanSegs / 64;
    __shared__ float PQ[kScanSegs][kScanCols][2];
    __shared__ double red[NWAVES][3];
    const long long C = a.C;
    const int T = a.T;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = lane & (W - 1), seg = (64 / W) * wave + lane / W;
    long long col = (long long)blockIdx.x * kScanCols + c;
    const bool live = col < C;
    if (!live) col = C - 1;
    const int Ls = (T + kScanSegs - 1) / kScanSegs;
    const int t0 = seg * Ls;
    int n = T - t0;
    if (n > Ls) n = Ls;
    if (n < 0) n = 0;
    const bool has_adv = a.adv != nullptr;
    float sigma, mu;
    load_denorm(a, DENORM, sigma, mu);
    const float gamma = a.gamma, gl = a.gl;

    // ---- 1. the whole segment into registers
    float r[kScanLmax], v0[kScanLmax], m1[kScanLmax], bad1[kScanLmax], am[kScanLmax];
    const float nv = a.next_value[col];
#pragma unroll
    for (int i = 0; i < kScanLmax; ++i) {
        const int t = t0 + (i < n ? i : 0);
        const long long o = (long long)(t < T ? t : 0) * C + col;
        r[i] = a.rewards[o];
        v0[i] = a.value_preds[o];
        m1[i] = a.masks[o + C];
        bad1[i] = PTL ? a.bad[o + C] : 1.f;
        am[i] = ACT ? a.active[o] : 1.f;
    }
    // D(v) of the step after the segment (the bootstrap value for the last one)
    float vend = nv;
    if (t0 + n < T) vend = a.value_preds[(long long)(t0 + n) * C + col];
    float dvend = vend;
    if (DENORM) {
        const float s = vend * sigma;
        dvend = s + mu;
    }
    if (seg == 0 && live) a.value_preds[(long long)T * C + col] = nv;      // shared_buffer.py:187,218

    // ---- 2. (P, Q) of the segment
    float P = 1.f, Q = 0.f;
    {
        float dv1 = dvend;
#pragma unroll
        for (int i = kScanLmax - 1; i >= 0; --i) {
            if (i < n) {
                float dv0 = v0[i];
                if (DENORM) {
                    const float s = v0[i] * sigma;
                    dv0 = s + mu;
                }
                const float delta = (r[i] + (gamma * dv1) * m1[i]) - dv0;
                float cc = gl * m1[i];
                float dd = delta;
                if (PTL) {
                    cc *= bad1[i];
                    dd *= bad1[i];
                }
                Q = dd + cc * Q;
                P = cc * P;
                dv1 = dv0;
            }
        }
    }
    PQ[seg][c][0] = P;
    PQ[seg][c][1] = Q;
    __syncthreads();
    // ---- 3. incoming g: the later segments composed from the end (g_T = 0)
    float g = 0.f;
    for (int s2 = kScanSegs - 1; s2 > seg; --s2) g = PQ[s2][c][1] + PQ[s2][c][0] * g;

    // ---- 4. the segment again, reference operation order
    double s1 = 0.0, sq = 0.0, cnt = 0.0;
    {
        float dv1 = dvend;
#pragma unroll
        for (int i = kScanLmax - 1; i >= 0; --i) {
            if (i < n) {
                float dv0;
                const float ret = gae_step<PTL, DENORM>(r[i], v0[i], m1[i], bad1[i], sigma, mu, gamma, gl, dv1, g, dv0);
                if (live) {
                    const long long o = (long long)(t0 + i) * C + col;
                    a.returns[o] = ret;
                    if (has_adv) {
                        const float adv = ret - dv0;
                        a.adv[o] = adv;
                        if (am[i] != 0.f) {
                            const double d = (double)adv;
                            s1 += d;
                            sq += d * d;
                            cnt += 1.0;
                        }
                    }
                }
            }
        }
    }
    zero_unowned_partials(a.partials, a.partial_rows);
    if (a.partials != nullptr) {
        s1 = wave_sum(s1);
        sq = wave_sum(sq);
        cnt = wave_sum(cnt);
        if (lane == 0) {
            red[wave][0] = s1;
            red[wave][1] = sq;
            red[wave][2] = cnt;
        }
        __syncthreads();
        if (threadIdx.x < 3) {
            double t = 0.0;
            for (int w = 0; w < NWAVES; ++w) t += red[w][threadIdx.x];
            a.partials[(long long)blockIdx.x * 3 + threadIdx.x] = t;
        }
    }
}

// ------------------------------------------------------- K5: moments and stats ----
__global__ void __launch_bounds__(256) adv_reduce_kernel(const double* partials, long long rows,
                                                          double* sums) {
    __shared__ double sh[3][256];
    double acc[3] = {0.0, 0.0, 0.0};
    for (long long r = threadIdx.x; r < rows; r += 256) {
        acc[0] += partials[r * 3 + 0];
        acc[1] += partials[r * 3 + 1];
        acc[2] += partials[r * 3 + 2];
    }
    for (int k = 0; k < 3; ++k) sh[k][threadIdx.x] = acc[k];
    __syncthreads();
    for (int stride = 128; stride > 0; stride >>= 1) {
        if ((int)threadIdx.x < stride)
            for (int k = 0; k < 3; ++k) sh[k][threadIdx.x] += sh[k][threadIdx.x + stride];
        __syncthreads();
    }
    if (threadIdx.x < 3) sums[threadIdx.x] = sh[threadIdx.x][0];
}

__global__ void adv_stats_kernel(const double* sums, float* stats) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        double n = sums[2];
        double mean = sums[0] / n;  // n == 0 -> NaN, like np.nanmean of an all-NaN array
        double var = sums[1] / n - mean * mean;
        if (var < 0.0) var = 0.0;
        stats[0] = (float)mean;
        stats[1] = (float)sqrt(var);
    }
}

__global__ void __launch_bounds__(256) adv_normalize_kernel(const float* adv, const float* stats,
                                                             float* out, long long n) {
    const float mean = stats[0];
    const float den = stats[1] + 1e-5f;  // r_mappo.py:187
    long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long step = (long long)gridDim.x * 256;
    for (; i < n; i += step) out[i] = (adv[i] - mean) / den;
}

constexpr int kAdvBlocks = 1024;

// r_mappo.py:179-186 as one grid-stride pass: advantages + per-block partial moments.
__global__ void __launch_bounds__(256) advantages_kernel(const float* ret, const float* vp,
                                                          const float* denorm, const float* active,
                                                          float* adv, double* partials, long long n,
                                                          long long partial_rows) {
    zero_unowned_partials(partials, partial_rows);
    float sigma = 1.f, mu = 0.f;
    const bool dn = denorm != nullptr;
    if (dn) {
        sigma = denorm[0];
        mu = denorm[1];
    }
    double s1 = 0.0, s2 = 0.0, cnt = 0.0;
    const long long step = (long long)gridDim.x * 256;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += step) {
        float dv = vp[i];
        if (dn) {
            float s = dv * sigma;
            dv = s + mu;
        }
        float a = ret[i] - dv;
        adv[i] = a;
        float am = active ? active[i] : 1.f;
        if (am != 0.f) {
            double d = (double)a;
            s1 += d;
            s2 += d * d;
            cnt += 1.0;
        }
    }
    __shared__ double sh[3][4];
    s1 = wave_sum(s1);
    s2 = wave_sum(s2);
    cnt = wave_sum(cnt);
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        sh[0][w] = s1;
        sh[1][w] = s2;
        sh[2][w] = cnt;
    }
    __syncthreads();
    if (threadIdx.x < 3 && partials)
        partials[(long long)blockIdx.x * 3 + threadIdx.x] =
            ((sh[threadIdx.x][0] + sh[threadIdx.x][1]) + sh[threadIdx.x][2]) + sh[threadIdx.x][3];
}

int g_variant = 0;
int g_last_variant = 0;

// Three runtime flags -> compile-time booleans: f(std::bool_constant<b0>, <b1>, <b2>) for the given values.  Every
// launcher below picks its template instance through this.
template <class F>
hipError_t with_flags(bool b0, bool b1, bool b2, F&& f) {
    using Y = std::true_type;
    using N = std::false_type;
    switch ((b0 ? 4 : 0) | (b1 ? 2 : 0) | (b2 ? 1 : 0)) {
        case 0: return f(N(), N(), N());
        case 1: return f(N(), N(), Y());
        case 2: return f(N(), Y(), N());
        case 3: return f(N(), Y(), Y());
        case 4: return f(Y(), N(), N());
        case 5: return f(Y(), N(), Y());
        case 6: return f(Y(), Y(), N());
        default: return f(Y(), Y(), Y());
    }
}

// (time limits, denorm, active masks) of a GAE launch
template <class F>
hipError_t with_gae_flags(const GaeArgs& a, unsigned flags, F&& f) {
    return with_flags(flags & MAPPO_GAE_PROPER_TIME_LIMITS, flags & MAPPO_GAE_DENORM, a.active != nullptr, f);
}

inline int gae_slots(const GaeArgs& a, unsigned flags) {
    return 3 + ((flags & MAPPO_GAE_PROPER_TIME_LIMITS) ? 1 : 0) + (a.active ? 1 : 0);
}

// Measurement hook (mappo_gae_time_next_launch): the next launch of an LDS-DMA ring kernel carries the library's own event
// pair AT DISPATCH LEVEL (hipExtLaunchKernelGGL: the events take the kernel's begin and end timestamps -- what rocprofv3's
// kernel trace reports).  A pair of hipEventRecord calls around the launch brackets two more packets of the command processor:
// + 5-6 us on this 50 us kernel, measured against the trace of the same run (profiles/r06_gae_in_situ_timing.json).
constexpr int kTimeSlots = 64;
hipEvent_t g_time_begin[kTimeSlots], g_time_end[kTimeSlots];
bool g_time_made[kTimeSlots], g_time_taken[kTimeSlots];
int g_time_armed = -1, g_time_next = 0;

// Launch of a ring kernel.  More than 64 KiB of dynamic LDS (gfx950 has 160 KiB per CU) is granted once per (device,
// kernel) by mappo::grant_lds, which keeps the attribute call out of every later launch.
template <typename K>
hipError_t launch_gae(K kernel, dim3 grid, dim3 block, size_t lds, hipStream_t stream, const GaeArgs& a) {
    if (lds > 64 * 1024) {
        const hipError_t e = mappo::grant_lds(kernel, lds);
        if (e != hipSuccess) return e;
    }
    if (g_time_armed >= 0) {
        const int s = g_time_armed;
        g_time_armed = -1;
        g_time_taken[s] = true;
        hipExtLaunchKernelGGL(kernel, grid, block, (uint32_t)lds, stream, g_time_begin[s], g_time_end[s], 0, a);
    } else {
        hipLaunchKernelGGL(kernel, grid, block, lds, stream, a);
    }
    return hipGetLastError();
}

template <int W, int NPROD, int TC, int R>
hipError_t launch_dma(const GaeArgs& a, unsigned flags, hipStream_t stream) {
    const size_t lds = (size_t)R * gae_slots(a, flags) * TC * W * sizeof(float);
    const dim3 grid((unsigned)((a.C + W - 1) / W)), block((NPROD + (W + 63) / 64) * 64);
    return with_gae_flags(a, flags, [&](auto ptl, auto den, auto act) {
        return launch_gae(gae_dma_kernel<W, NPROD, TC, R, ptl(), den(), act()>, grid, block, lds, stream, a);
    });
}

template <int W, int NPROD, int TC, int R>
hipError_t launch_dma_epi(const GaeArgs& a, unsigned flags, hipStream_t stream) {
    static_assert(epi_lds_bytes(R, 5, TC, W) <= 160 * 1024, "the ring must fit with all five input fields");
    const size_t lds = epi_lds_bytes(R, gae_slots(a, flags), TC, W);
    const dim3 grid((unsigned)((a.C + W - 1) / W)), block((NPROD + (W + 63) / 64) * 64);
    return with_gae_flags(a, flags, [&](auto ptl, auto den, auto act) {
        return launch_gae(gae_dma_epi_kernel<W, NPROD, TC, R, ptl(), den(), act()>, grid, block, lds, stream, a);
    });
}

template <int W>
hipError_t launch_scan(const GaeArgs& a, unsigned flags, hipStream_t stream) {
    const dim3 grid((unsigned)((a.C + W - 1) / W)), block(W * kScanSegs);
    return with_gae_flags(a, flags, [&](auto ptl, auto den, auto act) {
        hipLaunchKernelGGL((gae_scan_kernel<W, ptl(), den(), act()>), grid, block, 0, stream, a);
        return hipGetLastError();
    });
}

// ------------------------------------------------------------------- MAT kernel ----
// The multi-agent-transformer branches of compute_returns (shared_buffer.py:222-232 with a value
// normaliser, :241-248 without): GAE without time limits whose advantage output is the accumulator
// itself (advantages[t] = gae, not returns - D(v)), and -- without a normaliser -- whose TD error
// uses the mean over the env's agents of the value predictions.  One lane per column (n, a); the
// lanes of one env each form the group mean redundantly (A adjacent floats, served by L1).

// numpy's float32 add.reduce over a contiguous axis of n <= 128 elements (pairwise sum: plain loop
// below 8, eight interleaved partial sums up to 128; numpy/core/src/umath/loops_utils.h -- the
// recursive halving above 128 is not needed for agent counts and is rejected by the entry point).
constexpr int kMaxMatAgents = 128;
__device__ __forceinline__ float numpy_sum_f32(const float* a, int n) {
    if (n < 8) {
        float res = 0.f;
        for (int i = 0; i < n; ++i) res = res + a[i];
        return res;
    }
    {
        float r0 = a[0], r1 = a[1], r2 = a[2], r3 = a[3], r4 = a[4], r5 = a[5], r6 = a[6], r7 = a[7];
        int i = 8;
        for (; i < n - (n % 8); i += 8) {
            r0 = r0 + a[i + 0];
            r1 = r1 + a[i + 1];
            r2 = r2 + a[i + 2];
            r3 = r3 + a[i + 3];
            r4 = r4 + a[i + 4];
            r5 = r5 + a[i + 5];
            r6 = r6 + a[i + 6];
            r7 = r7 + a[i + 7];
        }
        float res = ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7));
        for (; i < n; ++i) res = res + a[i];
        return res;
    }
    return 0.f;
}

template <bool DENORM>
__global__ void __launch_bounds__(64) gae_mat_kernel(GaeArgs a, int A) {
    const long long C = a.C;
    const int T = a.T;
    const long long col = (long long)blockIdx.x * 64 + threadIdx.x;
    const bool live = col < C;
    const bool has_act = a.active != nullptr;
    float sigma, mu;
    load_denorm(a, DENORM, sigma, mu);
    const float gamma = a.gamma, gl = a.gl, fA = (float)A;
    double s1 = 0.0, s2 = 0.0, cnt = 0.0;
    if (live) {
        const long long g0 = (col / A) * A;  // first column of this env's agent group
        float nv = a.next_value[col];
        a.value_preds[(long long)T * C + col] = nv;  // shared_buffer.py:218
        float next_term;                             // D(v_{t+1}) or mean_a v_{t+1}
        if (DENORM) {
            float s = nv * sigma;
            next_term = s + mu;
        } else {
            next_term = numpy_sum_f32(a.next_value + g0, A) / fA;  // row T is being written: read the source
        }
        float g = 0.f;
        for (int t = T - 1; t >= 0; --t) {
            long long o = (long long)t * C + col;
            float r = a.rewards[o], v0 = a.value_preds[o], m1 = a.masks[o + C];
            float base = v0, cur_term;
            if (DENORM) {
                float s = v0 * sigma;
                base = s + mu;  // value_t (:223)
                cur_term = base;
            } else {
                cur_term = numpy_sum_f32(a.value_preds + (long long)t * C + g0, A) / fA;  // mean_v_t (:243)
            }
            float x = gamma * m1;  // :229 / :245: r + gamma * mask * next - cur
            float y = x * next_term;
            float z = r + y;
            float delta = z - cur_term;
            float c0 = gl * m1;  // :230 / :249
            float carry = c0 * g;
            g = delta + carry;
            a.adv[o] = g;               // :231 / :250
            a.returns[o] = g + base;    // :232 / :251
            next_term = cur_term;
            float am = has_act ? a.active[o] : 1.f;
            if (am != 0.f) {
                double d = (double)g;
                s1 += d;
                s2 += d * d;
                cnt += 1.0;
            }
        }
    }
    zero_unowned_partials(a.partials, a.partial_rows);
    write_partials(a, blockIdx.x, threadIdx.x, s1, s2, cnt);
}

hipError_t launch_column(const GaeArgs& a, unsigned flags, hipStream_t stream) {
    const dim3 grid((unsigned)((a.C + 63) / 64)), block(64);
    // (without GAE, D() only enters the fused advantages)
    return with_flags(flags & MAPPO_GAE_USE_GAE, flags & MAPPO_GAE_PROPER_TIME_LIMITS, flags & MAPPO_GAE_DENORM,
                      [&](auto gae, auto ptl, auto den) {
                          hipLaunchKernelGGL((gae_column_kernel<gae(), ptl(), den()>), grid, block, 0, stream, a);
                          return hipGetLastError();
                      });
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

}  // namespace

extern "C" int64_t mappo_gae_partial_rows(int64_t C) {
    if (C <= 0) return 0;
    int64_t r = (C + 15) / 16;
    return r < kAdvBlocks ? kAdvBlocks : r;
}

extern "C" int mappo_advantages_f32(const float* returns, const float* value_preds,
                                    const float* denorm, const float* active_masks,
                                    float* advantages, double* adv_partials, int T, int64_t C,
                                    mappo_stream_t stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (!returns || !value_preds || !advantages) return MAPPO_E_NULL;
    if (T <= 0 || C <= 0) return MAPPO_E_SHAPE;
    const long long n = (long long)T * C;
    long long blocks = (n + 256 * 8 - 1) / (256 * 8);
    if (blocks > kAdvBlocks) blocks = kAdvBlocks;
    hipLaunchKernelGGL(advantages_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, returns,
                       value_preds, denorm, active_masks, advantages, adv_partials, n,
                       (long long)mappo_gae_partial_rows(C));
    return (int)hipGetLastError();
}

extern "C" int mappo_gae_set_variant(int variant) {
    int old = g_variant;
    g_variant = variant;
    return old;
}

extern "C" int mappo_gae_last_variant(void) { return g_last_variant; }

extern "C" int mappo_gae_time_next_launch(void) {
    const int s = g_time_next;
    if (!g_time_made[s]) {
        if (hipEventCreate(&g_time_begin[s]) != hipSuccess || hipEventCreate(&g_time_end[s]) != hipSuccess) return MAPPO_E_FLAGS;
        g_time_made[s] = true;
    }
    g_time_next = (s + 1) % kTimeSlots;
    g_time_taken[s] = false;
    g_time_armed = s;
    return s;
}

extern "C" int mappo_gae_timed_launch_ms(int slot, float* ms) {
    if (!ms) return MAPPO_E_NULL;
    if (slot < 0 || slot >= kTimeSlots) return MAPPO_E_SHAPE;
    if (g_time_armed == slot) g_time_armed = -1;                            // (asked before any launch took it: disarmed)
    if (!g_time_made[slot] || !g_time_taken[slot]) return MAPPO_E_FLAGS;    // never armed, or the armed call took a kernel without the hook
    if (hipEventSynchronize(g_time_end[slot]) != hipSuccess) return (int)hipGetLastError();
    return (int)hipEventElapsedTime(ms, g_time_begin[slot], g_time_end[slot]);
}

extern "C" int mappo_gae_f32(const float* rewards, float* value_preds, const float* next_value,
                             const float* masks, const float* bad_masks, float* returns,
                             const float* denorm, float* advantages, const float* active_masks,
                             double* adv_partials, int T, int64_t C, double gamma,
                             double gae_lambda, unsigned flags, mappo_stream_t stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (!rewards || !value_preds || !next_value || !masks || !returns) return MAPPO_E_NULL;
    if ((flags & MAPPO_GAE_PROPER_TIME_LIMITS) && !bad_masks) return MAPPO_E_NULL;
    if ((flags & MAPPO_GAE_DENORM) && !denorm) return MAPPO_E_NULL;
    if (flags & ~15u) return MAPPO_E_FLAGS;
    if (T <= 0 || C <= 0) return MAPPO_E_SHAPE;
    if (adv_partials && !advantages) return MAPPO_E_NULL;
    if (active_masks && !advantages) return MAPPO_E_NULL;
    const void* ptrs[] = {rewards, value_preds, next_value, masks, bad_masks, returns,
                          denorm,  advantages,  active_masks};
    for (const void* p : ptrs)
        if (p && (reinterpret_cast<uintptr_t>(p) & 3u)) return MAPPO_E_ALIGN;

    GaeArgs a;
    a.rewards = rewards;
    a.value_preds = value_preds;
    a.next_value = next_value;
    a.masks = masks;
    a.bad = (flags & MAPPO_GAE_PROPER_TIME_LIMITS) ? bad_masks : nullptr;
    a.returns = returns;
    a.denorm = (flags & MAPPO_GAE_DENORM) ? denorm : nullptr;
    a.adv = advantages;
    a.active = active_masks;
    a.partials = adv_partials;
    a.partial_rows = mappo_gae_partial_rows(C);
    a.T = T;
    a.C = C;
    a.gamma = (float)gamma;
    a.gl = (float)(gamma * gae_lambda);

    const bool strip_ok = (flags & MAPPO_GAE_USE_GAE) && (C % 4 == 0) && C >= 4 && aligned16(rewards) &&
                          aligned16(value_preds) && aligned16(masks) &&
                          (!a.bad || aligned16(bad_masks)) && (!a.active || aligned16(active_masks));
    int variant = g_variant % 1000;
    a.opts = g_variant / 1000;
    if (!strip_ok) variant = 99;
    // narrow buffers: the time-parallel scan (tolerance mode) unless the caller insists on bit-exact results
    const bool scan_ok = strip_ok && T <= kScanSegs * kScanLmax && (!a.partials || a.partial_rows >= (C + 31) / 32);
    if (variant == 71 || variant == 72) variant = 70;   // the 64- and 16-column scans are gone: aliases of the one that is built
    if (variant == 70 && !scan_ok) variant = 0;
    if (variant == 0 && scan_ok && !(flags & MAPPO_GAE_EXACT) && C >= 2048 && C < 16384 && T >= 64) variant = 70;
    if (variant == 0) {
        // LDS-DMA ring kernel; strip width by column count so that >= 256 workgroups exist;
        // XCD-contiguous strip order + non-temporal DMA (measured best on cold data)
        variant = (C >= 128 * 256) ? 57 : (C >= 64 * 256) ? 54 : (C >= 32 * 256 ? 56 : 36);
        a.opts = 3;
    }

    g_last_variant = variant;
    // The kernels the automatic choice can reach, plus 99 for the column kernel.  Any other number -- among them those of
    // the tuning variants that are no longer built -- has no case and runs the column kernel.
    switch (variant) {
        // LDS-DMA ring, walker does the epilogue
        case 36: return (int)launch_dma<16, 1, 16, 4>(a, flags, stream);
        // LDS-DMA ring, epilogue on the producer waves
        case 54: return (int)launch_dma_epi<64, 2, 16, 4>(a, flags, stream);
        case 56: return (int)launch_dma_epi<32, 2, 16, 4>(a, flags, stream);
        case 57: return (int)launch_dma_epi<128, 6, 12, 4>(a, flags, stream);
        case 70: return (int)launch_scan<32>(a, flags, stream);
        default: return (int)launch_column(a, flags, stream);
    }
}

extern "C" int mappo_gae_mat_f32(const float* rewards, float* value_preds, const float* next_value,
                                 const float* masks, float* returns, const float* denorm,
                                 float* advantages, const float* active_masks, double* adv_partials,
                                 int T, int64_t C, int num_agents, double gamma, double gae_lambda,
                                 unsigned flags, mappo_stream_t stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (!rewards || !value_preds || !next_value || !masks || !returns || !advantages) return MAPPO_E_NULL;
    if ((flags & MAPPO_GAE_DENORM) && !denorm) return MAPPO_E_NULL;
    if (flags & ~MAPPO_GAE_DENORM) return MAPPO_E_FLAGS;
    if (T <= 0 || C <= 0 || num_agents <= 0 || C % num_agents != 0) return MAPPO_E_SHAPE;
    if (!(flags & MAPPO_GAE_DENORM) && num_agents > kMaxMatAgents) return MAPPO_E_TOO_MANY;
    const void* ptrs[] = {rewards, value_preds, next_value, masks, returns, denorm, advantages, active_masks};
    for (const void* p : ptrs)
        if (p && (reinterpret_cast<uintptr_t>(p) & 3u)) return MAPPO_E_ALIGN;
    GaeArgs a;
    a.rewards = rewards;
    a.value_preds = value_preds;
    a.next_value = next_value;
    a.masks = masks;
    a.bad = nullptr;
    a.returns = returns;
    a.denorm = (flags & MAPPO_GAE_DENORM) ? denorm : nullptr;
    a.adv = advantages;
    a.active = active_masks;
    a.partials = adv_partials;
    a.partial_rows = mappo_gae_partial_rows(C);
    a.opts = 0;
    a.T = T;
    a.C = C;
    a.gamma = (float)gamma;
    a.gl = (float)(gamma * gae_lambda);
    dim3 grid((unsigned)((C + 63) / 64)), block(64);
    if (flags & MAPPO_GAE_DENORM)
        hipLaunchKernelGGL((gae_mat_kernel<true>), grid, block, 0, stream, a, num_agents);
    else
        hipLaunchKernelGGL((gae_mat_kernel<false>), grid, block, 0, stream, a, num_agents);
    return (int)hipGetLastError();
}

extern "C" int mappo_adv_reduce(const double* partials, int64_t rows, double* sums,
                                mappo_stream_t stream_) {
    if (!partials || !sums) return MAPPO_E_NULL;
    if (rows <= 0) return MAPPO_E_SHAPE;
    hipLaunchKernelGGL(adv_reduce_kernel, dim3(1), dim3(256), 0, static_cast<hipStream_t>(stream_),
                       partials, (long long)rows, sums);
    return (int)hipGetLastError();
}

extern "C" int mappo_adv_stats(const double* sums, float* stats, mappo_stream_t stream_) {
    if (!sums || !stats) return MAPPO_E_NULL;
    hipLaunchKernelGGL(adv_stats_kernel, dim3(1), dim3(64), 0, static_cast<hipStream_t>(stream_),
                       sums, stats);
    return (int)hipGetLastError();
}

extern "C" int mappo_adv_normalize(const float* adv, const float* stats, float* out, int64_t n,
                                   mappo_stream_t stream_) {
    if (!adv || !stats || !out) return MAPPO_E_NULL;
    if (n <= 0) return MAPPO_E_SHAPE;
    long long blocks = (n + 255) / 256;
    if (blocks > 256 * 16) blocks = 256 * 16;
    hipLaunchKernelGGL(adv_normalize_kernel, dim3((unsigned)blocks), dim3(256), 0,
                       static_cast<hipStream_t>(stream_), adv, stats, out, (long long)n);
    return (int)hipGetLastError();
}
