// K17: the turn bookkeeping of a Hanabi move on the device (C ABI and reference file:line: include/mappo_hip.h, "K17").
//
// Two launches around K16's env step.  Everything they decide they read off device memory -- can_move (bit 8 of the flags
// words of the previous call) and the status byte of the flags words of this one -- so a move of the turn-based runner
// needs no device -> host copy and can be replayed from a captured graph.
//
// Shape of both kernels: ONE WAVE per table, four waves a workgroup, at most MAPPO_TURN_MAX_BLOCKS workgroups that stride
// over the tables.  Lane 0 does the table's scalar work (a dozen words); all 64 lanes move or clear the table's rows.  A
// row of width W starts at (row index) * W floats: 16-byte aligned only when that product is a multiple of four, so rows
// are written as aligned float4 between a scalar head and a scalar tail (the idiom of stream_row in mappo_hanabi.hip), and
// read as float4 too when the source row sits at the same offset from a 16-byte boundary as the destination row (else as
// four dwords: still consecutive lanes on consecutive addresses).  No LDS, no atomics, nothing allocated.
//
// K17 for a recurrent policy (mappo_hanabi_turn_begin_rnn / _end_rnn): the same two kernels, instantiated on a descriptor that
// also carries the actor's and the critic's RNN state per (table, player) -- the movers' new states go into slot `agent`, a
// finished table's states are cleared for every player.
//
// K18: the same two launches for an EVALUATION move (include/mappo_hip.h, "K18"): no buffer slots, rewards or masks, but the
// actor's RNN state per (table, player), a final score per table, and finished tables that never restart.  Same shape, same
// row helpers.
#include "mappo_internal.h"
#include "../../include/mappo_hip.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kStatusDone = 1, kStatusRefused = 255;

// dst[d0 .. d0 + w) = src[s0 .. s0 + w); dst and src are 16-byte aligned arrays, d0 / s0 float offsets of the rows.
__device__ __forceinline__ void copy_row(float* dst, size_t d0, const float* src, size_t s0, int w, int lane) {
    const int shift = (int)(d0 & 3);
    float* base = dst + (d0 - shift);               // 16-byte aligned; element k of it is row element k - shift
    const float* from = src + s0;
    const bool same_phase = (int)(s0 & 3) == shift;  // wave-uniform
    const int end = shift + w, nvec = (end + 3) / 4;
    for (int v = lane; v < nvec; v += 64) {
        const int lo = v * 4;
        if (lo >= shift && lo + 4 <= end) {
            const float* p = from + (lo - shift);
            float4 x;
            if (same_phase) x = *reinterpret_cast<const float4*>(p);
            else x = make_float4(p[0], p[1], p[2], p[3]);
            *reinterpret_cast<float4*>(base + lo) = x;
        } else {
            for (int k = lo; k < lo + 4; ++k)
                if (k >= shift && k < end) base[k] = from[k - shift];
        }
    }
}

// dst[d0 .. d0 + w) = 0
__device__ __forceinline__ void zero_row(float* dst, size_t d0, int w, int lane) {
    const int shift = (int)(d0 & 3);
    float* base = dst + (d0 - shift);
    const int end = shift + w, nvec = (end + 3) / 4;
    for (int v = lane; v < nvec; v += 64) {
        const int lo = v * 4;
        if (lo >= shift && lo + 4 <= end) {
            *reinterpret_cast<float4*>(base + lo) = make_float4(0.f, 0.f, 0.f, 0.f);
        } else {
            for (int k = lo; k < lo + 4; ++k)
                if (k >= shift && k < end) base[k] = 0.f;
        }
    }
}

// The training move's two kernels stand once, for both descriptors: D = mappo_hanabi_turn_t (K17) or mappo_hanabi_turn_rnn_t
// (the same fields in front, then the carried RNN states of a recurrent policy).  What kRnn guards is compiled into the
// second instantiation only.
template <typename D> constexpr bool kRnn = false;
template <> constexpr bool kRnn<mappo_hanabi_turn_rnn_t> = true;

template <typename D>
__global__ void __launch_bounds__(kThreads) hanabi_turn_begin_kernel(D d, int agent) {
    const int lane = threadIdx.x & 63;
    const long long first = (long long)blockIdx.x * kWaves + (threadIdx.x >> 6), step = (long long)gridDim.x * kWaves;
    const size_t A = (size_t)d.players;
    for (long long n = first; n < d.n_tables; n += step) {
        const bool m = d.can_move[n] != 0;           // one address per wave
        if (lane == 0) d.env_actions[n] = m ? (int32_t)d.action[n] : -1;
        if (!m) continue;
        const size_t slot = (size_t)n * A + (size_t)agent;
        if (lane == 0) {
            d.values[slot] = d.value[n];
            d.actions[slot] = (float)d.action[n];
            d.action_log_probs[slot] = d.logp[n];
        }
        copy_row(d.obs, slot * d.obs_w, d.use_obs, (size_t)n * d.obs_w, d.obs_w, lane);
        copy_row(d.share_obs, slot * d.share_w, d.use_share_obs, (size_t)n * d.share_w, d.share_w, lane);
        copy_row(d.available_actions, slot * d.avail_w, d.use_available_actions, (size_t)n * d.avail_w, d.avail_w, lane);
        if constexpr (kRnn<D>) {
            copy_row(d.rnn_states, slot * d.rnn_w, d.rnn_new, (size_t)n * d.rnn_w, d.rnn_w, lane);
            copy_row(d.rnn_states_critic, slot * d.rnn_w, d.rnn_new_critic, (size_t)n * d.rnn_w, d.rnn_w, lane);
        }
    }
}

template <typename D>
__global__ void __launch_bounds__(kThreads) hanabi_turn_end_kernel(D d, int agent) {
    const int lane = threadIdx.x & 63;
    const long long first = (long long)blockIdx.x * kWaves + (threadIdx.x >> 6), step = (long long)gridDim.x * kWaves;
    const int A = d.players;
    float* rsla = d.rewards_since_last_action;
    for (long long n = first; n < d.n_tables; n += step) {
        const int32_t f = d.flags[n];
        const int status = f & 0xff;
        const bool done = status == kStatusDone;
        const size_t row = (size_t)n * (size_t)A;
        if (lane == 0) {
            const size_t slot = row + (size_t)agent;
            if (d.can_move[n] != 0) {
                d.rewards[slot] = rsla[slot];
                rsla[slot] = 0.f;
                const float r = d.rewards_env[n];
                for (int a = 0; a < A; ++a) rsla[row + a] += r;
                d.moves[n] += 1;
            }
            if (status == 0) d.masks[slot] = d.active_masks[slot] = 1.f;
            if (done) {
                d.reset_choose[n] = 1;
                d.games[n] += 1;
                d.score_sum[n] += f >> 16;
                for (int a = 0; a < A; ++a) d.masks[row + a] = 0.f;
                d.active_masks[slot] = 1.f;
                for (int a = agent + 1; a < A; ++a) {
                    d.active_masks[row + a] = 0.f;
                    d.rewards[row + a] = rsla[row + a];
                    rsla[row + a] = 0.f;
                    d.values[row + a] = 0.f;
                }
            }
            if (status == kStatusRefused) d.refused[n] = 1;
            d.can_move[n] = done ? 0 : (f >> 8) & 1;
        }
        if (!done) continue;
        zero_row(d.use_available_actions, (size_t)n * d.avail_w, d.avail_w, lane);
        for (int a = agent + 1; a < A; ++a) {
            zero_row(d.obs, (row + a) * d.obs_w, d.obs_w, lane);
            zero_row(d.share_obs, (row + a) * d.share_w, d.share_w, lane);
        }
        if constexpr (kRnn<D>) {
            // every player's state restarts with the game: the A slot rows of a table are one stretch of A * rnn_w floats
            zero_row(d.rnn_states, row * d.rnn_w, A * d.rnn_w, lane);
            zero_row(d.rnn_states_critic, row * d.rnn_w, A * d.rnn_w, lane);
        }
    }
}

__global__ void __launch_bounds__(kThreads) hanabi_eval_begin_kernel(mappo_hanabi_eval_t d, int agent) {
    const int lane = threadIdx.x & 63;
    const long long first = (long long)blockIdx.x * kWaves + (threadIdx.x >> 6), step = (long long)gridDim.x * kWaves;
    const size_t A = (size_t)d.players;
    for (long long n = first; n < d.n_tables; n += step) {
        const bool m = d.can_move[n] != 0;           // one address per wave
        if (lane == 0) d.env_actions[n] = m ? (int32_t)d.action[n] : -1;
        if (!m || !d.rnn_states) continue;
        copy_row(d.rnn_states, ((size_t)n * A + (size_t)agent) * d.rnn_w, d.rnn_new, (size_t)n * d.rnn_w, d.rnn_w, lane);
    }
}

__global__ void __launch_bounds__(kThreads) hanabi_eval_end_kernel(mappo_hanabi_eval_t d, int agent) {
    const int lane = threadIdx.x & 63;
    const long long first = (long long)blockIdx.x * kWaves + (threadIdx.x >> 6), step = (long long)gridDim.x * kWaves;
    for (long long n = first; n < d.n_tables; n += step) {
        const int32_t f = d.flags[n];
        const int status = f & 0xff;
        // can_move[n] is read and rewritten by lane 0 alone; whether the table just finished reaches the other lanes
        // (which clear its legal-move row) from lane 0's registers, not through memory
        const bool m = lane == 0 && d.can_move[n] != 0;
        const bool done = m && status == kStatusDone;
        const bool done_u = __shfl((int)done, 0) != 0;
        if (lane == 0) {
            if (m) d.moves[n] += 1;
            if (done) {
                d.scores[n] = f >> 16;
                d.games[n] += 1;
            }
            if (status == kStatusRefused) d.refused[n] = 1;
            d.can_move[n] = (m && status == 0) ? (f >> 8) & 1 : 0;
        }
        if (done_u) zero_row(d.use_available_actions, (size_t)n * d.avail_w, d.avail_w, lane);
    }
}

unsigned grid_of(long long n) {
    const long long blocks = (n + kWaves - 1) / kWaves;
    return (unsigned)(blocks < MAPPO_TURN_MAX_BLOCKS ? blocks : MAPPO_TURN_MAX_BLOCKS);
}

// `used`: the pointers this entry point reads or writes (the other one's may be NULL).
template <typename D, size_t K>
int check(const D* d, int agent, const void* const (&used)[K]) {
    for (const void* p : used)
        if (!p) return MAPPO_E_NULL;
    if (d->n_tables <= 0 || d->players < 1 || d->players > MAPPO_TURN_MAX_PLAYERS || agent < 0 || agent >= d->players ||
        d->obs_w <= 0 || d->share_w <= 0 || d->avail_w <= 0)
        return MAPPO_E_SHAPE;
    if constexpr (kRnn<D>)
        if (d->rnn_w <= 0 || d->rnn_w > INT32_MAX / MAPPO_TURN_MAX_PLAYERS) return MAPPO_E_SHAPE;    // (players * rnn_w: an int)
    const void* rows[] = {d->obs, d->share_obs, d->available_actions, d->use_obs, d->use_share_obs, d->use_available_actions};
    for (const void* p : rows)
        if (!mappo::aligned_to(p, 16)) return MAPPO_E_ALIGN;
    if constexpr (kRnn<D>) {
        const void* states[] = {d->rnn_states, d->rnn_states_critic, d->rnn_new, d->rnn_new_critic};
        for (const void* p : states)
            if (!mappo::aligned_to(p, 16)) return MAPPO_E_ALIGN;
    }
    if (!mappo::aligned_to(d->moves, 8) || !mappo::aligned_to(d->action, 8)) return MAPPO_E_ALIGN;
    const void* words[] = {d->values, d->actions, d->action_log_probs, d->rewards, d->rewards_since_last_action, d->masks,
                           d->active_masks, d->value, d->logp, d->flags, d->rewards_env, d->can_move, d->env_actions,
                           d->games, d->score_sum};
    for (const void* p : words)
        if (!mappo::aligned_to(p, 4)) return MAPPO_E_ALIGN;
    return 0;
}

template <typename D, size_t K>
int enqueue(void (*kernel)(D, int), const D* d, int agent, const void* const (&used)[K], mappo_stream_t stream_) {
    const int rc = check(d, agent, used);
    if (rc != 0) return rc;
    hipLaunchKernelGGL(kernel, dim3(grid_of(d->n_tables)), dim3(kThreads), 0, static_cast<hipStream_t>(stream_), *d, agent);
    return (int)hipGetLastError();
}

template <size_t K>
int check_eval(const mappo_hanabi_eval_t* d, int agent, const void* const (&used)[K]) {
    for (const void* p : used)
        if (!p) return MAPPO_E_NULL;
    if ((d->rnn_states == nullptr) != (d->rnn_new == nullptr)) return MAPPO_E_NULL;
    if (d->n_tables <= 0 || d->players < 1 || d->players > MAPPO_TURN_MAX_PLAYERS || agent < 0 || agent >= d->players ||
        d->avail_w <= 0 || (d->rnn_states && d->rnn_w <= 0))
        return MAPPO_E_SHAPE;
    const void* rows[] = {d->use_available_actions, d->rnn_states, d->rnn_new};
    for (const void* p : rows)
        if (!mappo::aligned_to(p, 16)) return MAPPO_E_ALIGN;
    if (!mappo::aligned_to(d->moves, 8) || !mappo::aligned_to(d->action, 8)) return MAPPO_E_ALIGN;
    const void* words[] = {d->flags, d->can_move, d->env_actions, d->games, d->scores};
    for (const void* p : words)
        if (!mappo::aligned_to(p, 4)) return MAPPO_E_ALIGN;
    return 0;
}

}  // namespace

// the pointers the begin / end operation reads or writes, whichever descriptor carries them
#define TURN_BEGIN_USES(d) d.obs, d.share_obs, d.available_actions, d.values, d.actions, d.action_log_probs, d.use_obs, \
                           d.use_share_obs, d.use_available_actions, d.value, d.action, d.logp, d.can_move, d.env_actions
#define TURN_END_USES(d) d.obs, d.share_obs, d.values, d.rewards, d.rewards_since_last_action, d.masks, d.active_masks, \
                         d.use_available_actions, d.flags, d.rewards_env, d.can_move, d.reset_choose, d.moves, d.games, \
                         d.score_sum, d.refused

extern "C" int mappo_hanabi_turn_begin(const mappo_hanabi_turn_t* args, int agent, mappo_stream_t stream_) {
    if (!args) return MAPPO_E_NULL;
    const mappo_hanabi_turn_t& d = *args;
    const void* const used[] = {TURN_BEGIN_USES(d)};
    return enqueue(hanabi_turn_begin_kernel<mappo_hanabi_turn_t>, args, agent, used, stream_);
}

extern "C" int mappo_hanabi_turn_end(const mappo_hanabi_turn_t* args, int agent, mappo_stream_t stream_) {
    if (!args) return MAPPO_E_NULL;
    const mappo_hanabi_turn_t& d = *args;
    const void* const used[] = {TURN_END_USES(d)};
    return enqueue(hanabi_turn_end_kernel<mappo_hanabi_turn_t>, args, agent, used, stream_);
}

extern "C" int mappo_hanabi_turn_begin_rnn(const mappo_hanabi_turn_rnn_t* args, int agent, mappo_stream_t stream_) {
    if (!args) return MAPPO_E_NULL;
    const mappo_hanabi_turn_rnn_t& d = *args;
    const void* const used[] = {TURN_BEGIN_USES(d), d.rnn_states, d.rnn_states_critic, d.rnn_new, d.rnn_new_critic};
    return enqueue(hanabi_turn_begin_kernel<mappo_hanabi_turn_rnn_t>, args, agent, used, stream_);
}

extern "C" int mappo_hanabi_turn_end_rnn(const mappo_hanabi_turn_rnn_t* args, int agent, mappo_stream_t stream_) {
    if (!args) return MAPPO_E_NULL;
    const mappo_hanabi_turn_rnn_t& d = *args;
    const void* const used[] = {TURN_END_USES(d), d.rnn_states, d.rnn_states_critic};
    return enqueue(hanabi_turn_end_kernel<mappo_hanabi_turn_rnn_t>, args, agent, used, stream_);
}

extern "C" int mappo_hanabi_eval_begin(const mappo_hanabi_eval_t* args, int agent, mappo_stream_t stream_) {
    if (!args) return MAPPO_E_NULL;
    const mappo_hanabi_eval_t& d = *args;
    const void* const used[] = {d.action, d.can_move, d.env_actions};
    const int rc = check_eval(args, agent, used);
    if (rc != 0) return rc;
    hipLaunchKernelGGL(hanabi_eval_begin_kernel, dim3(grid_of(args->n_tables)), dim3(kThreads), 0,
                       static_cast<hipStream_t>(stream_), *args, agent);
    return (int)hipGetLastError();
}

extern "C" int mappo_hanabi_eval_end(const mappo_hanabi_eval_t* args, int agent, mappo_stream_t stream_) {
    if (!args) return MAPPO_E_NULL;
    const mappo_hanabi_eval_t& d = *args;
    const void* const used[] = {d.use_available_actions, d.flags, d.can_move, d.moves, d.games, d.scores, d.refused};
    const int rc = check_eval(args, agent, used);
    if (rc != 0) return rc;
    hipLaunchKernelGGL(hanabi_eval_end_kernel, dim3(grid_of(args->n_tables)), dim3(kThreads), 0,
                       static_cast<hipStream_t>(stream_), *args, agent);
    return (int)hipGetLastError();
}
