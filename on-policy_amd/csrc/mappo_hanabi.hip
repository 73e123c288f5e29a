// K16: Hanabi tables on the device (C ABI and reference file:line: include/mappo_hip.h, "K16").
//
// The rules, the deal and the encoder sections are hanabi_rules.h -- the code libhanabi_batch.so runs on the host.
// What is device-specific is the state layout and the two kernel shapes of a move:
//
//   apply / deal   one THREAD per table.  The generator's 624 words lie [624][N] (word k of table n at mt[k * N + n]), so
//                  the tables of a wave touch neighbouring words; the ~230-byte game PODs are array-of-structs behind
//                  them.  The thread validates the move, applies it, deals, and writes reward / status / score and the
//                  flags word (status | can-move << 8 | score << 16) -- the one thing the host reads back per move.
//   encode         one WORKGROUP per table: the row image [observation | turn] [centralised row] [legal moves] is
//                  cleared in LDS, the lanes set the ones (one lane per unit of an encoded view -- a hand, the board,
//                  the discards, the last move, a slot of the card knowledge -- and one per move uid: no two lanes
//                  store to one address), and all lanes stream the image out 16 bytes per lane.  A row starts
//                  at table * width floats, 16-byte aligned only every fourth table, so each row sits in LDS shifted
//                  by its global misalignment: aligned float4 of the image <-> aligned float4 of the output array, and
//                  only a row's first and last partial float4 go out as scalars.
//
// Nothing here allocates; every index is bounded by the rules (validated on the host) and the kMax* constants.
#include "mappo_internal.h"
#include "../../include/mappo_hip.h"
#include "hanabi_rules.h"

namespace {

using namespace hanabi;

constexpr int kMtWords = 624;
constexpr int kEncodeThreads = 256;
constexpr long long kMaxTables = 1ll << 24;
constexpr size_t kMaxImageBytes = 48 * 1024;         // LDS a kernel gets without a grant
constexpr int kStatusRefused = 255;
constexpr int kOk = 0;

struct DeviceTable {
    Game g;
    uint32_t mt_idx, drawn;
};

struct State {               // caller's buffer of n * mappo_hanabi_state_bytes(): [624][n] words, then n DeviceTable
    uint32_t* mt;
    DeviceTable* tab;
    long long n;
};

State carve(void* state, long long n) {
    uint32_t* mt = static_cast<uint32_t*>(state);
    return State{mt, reinterpret_cast<DeviceTable*>(mt + (size_t)kMtWords * (size_t)n), n};
}

__device__ __forceinline__ MtChance chance_of(const State& s, long long i) {
    return MtChance{Mt19937Strided{s.mt + i, (size_t)s.n, &s.tab[i].mt_idx, &s.tab[i].drawn}};
}

__device__ __forceinline__ int can_move(const Layout& L, const Game& g) {
    for (int u = 0; u < L.num_moves; ++u)
        if (legal(L, g, move_of(L, u))) return 1;
    return 0;
}

__device__ __forceinline__ int flags_word(int status, int movable, int score) {
    return status | (movable << 8) | (score << 16);
}

__global__ void __launch_bounds__(64) hanabi_seed_kernel(State s, const int32_t* seeds) {
    const long long i = (long long)blockIdx.x * 64 + threadIdx.x;
    if (i >= s.n) return;
    DeviceTable* t = &s.tab[i];
    uint32_t* words = reinterpret_cast<uint32_t*>(t);
    for (unsigned k = 0; k < sizeof(DeviceTable) / 4; ++k) words[k] = 0;      // started = false
    mt_seed(s.mt + i, (size_t)s.n, (uint32_t)seeds[i], &t->mt_idx, &t->drawn);
}

__global__ void __launch_bounds__(64) hanabi_deal_kernel(State s, Layout L, const uint8_t* choose, int32_t* flags) {
    const long long i = (long long)blockIdx.x * 64 + threadIdx.x;
    if (i >= s.n) return;
    Game* g = &s.tab[i].g;
    if (choose[i]) {
        MtChance chance = chance_of(s, i);
        new_game(L, g, chance);
        flags[i] = flags_word(0, can_move(L, *g), score_of(L, *g));
    } else {
        flags[i] = flags_word(2, 0, g->started && consistent(L, *g) ? score_of(L, *g) : 0);
    }
}

__global__ void __launch_bounds__(64) hanabi_apply_kernel(State s, Layout L, const int32_t* actions, float* rewards,
                                                          uint8_t* status, int32_t* scores, int32_t* flags) {
    const long long i = (long long)blockIdx.x * 64 + threadIdx.x;
    if (i >= s.n) return;
    Game* g = &s.tab[i].g;
    const int uid = actions[i];
    float reward = 0.0f;
    const bool usable = g->started && consistent(L, *g);
    int st, movable = 0, score = usable ? score_of(L, *g) : 0;
    if (!usable) {
        st = kStatusRefused;
    } else if (uid == -1) {
        st = 2;
    } else {
        const Move m = move_of(L, uid);              // kNone for a uid out of range, never legal
        if (!legal(L, *g, m)) {
            st = kStatusRefused;                     // the table stays as it was
        } else {
            MtChance chance = chance_of(s, i);
            apply(L, g, m, chance);
            const int after = score_of(L, *g);
            reward = (float)(after - score);
            score = after;
            st = end_of(L, *g) != kRunning ? 1 : 0;
            movable = can_move(L, *g);
        }
    }
    rewards[i] = reward;
    status[i] = (uint8_t)st;
    scores[i] = score;
    flags[i] = flags_word(st, movable, score);
}

__global__ void __launch_bounds__(64) hanabi_draws_kernel(State s, int32_t* out) {
    const long long i = (long long)blockIdx.x * 64 + threadIdx.x;
    if (i < s.n) out[i] = (int32_t)s.tab[i].drawn;
}

// ------------------------------------------------------------------------------------------------ encoder
struct Rows {
    float *obs, *share, *avail;
    int32_t* to_move;
    int obs_w, share_w, avail_w;         // floats per row
    int obs_at, share_at, avail_at;      // float offsets of the three regions in the LDS image (multiples of 4)
    int image_floats;                    // multiple of 4
    int share_mode;
};

__host__ __device__ inline int region_floats(int w) { return (w + 3 + 3) / 4 * 4; }     // a row shifted by up to 3 floats

// Region `lds` (16-byte aligned) holds a row at lds + (g0 & 3); out[g0 .. g0 + w) receives it.
__device__ __forceinline__ void stream_row(float* out, size_t g0, int w, const float* lds) {
    const int shift = (int)(g0 & 3);
    float* base = out + (g0 - shift);                // 16-byte aligned: out is, and g0 - shift is a multiple of 4
    const int end = shift + w, nvec = (end + 3) / 4;
    for (int v = threadIdx.x; v < nvec; v += kEncodeThreads) {
        const int lo = v * 4;
        if (lo >= shift && lo + 4 <= end) {
            *reinterpret_cast<float4*>(base + lo) = *reinterpret_cast<const float4*>(lds + lo);
        } else {
            for (int k = lo; k < lo + 4; ++k)
                if (k >= shift && k < end) base[k] = lds[k];
        }
    }
}

// active == NULL: a table takes part when its flags word says it moved (status 0 or 1); flags == NULL too: all do.
__global__ void __launch_bounds__(kEncodeThreads)
hanabi_encode_kernel(State s, Layout L, Rows r, const uint8_t* active, const int32_t* flags) {
    extern __shared__ float4 image4[];
    __shared__ DeviceTable held;
    float* image = reinterpret_cast<float*>(image4);
    const long long i = blockIdx.x;
    const int tid = threadIdx.x;

    for (int v = tid; v < r.image_floats / 4; v += kEncodeThreads) image4[v] = make_float4(0.f, 0.f, 0.f, 0.f);
    const uint32_t* src = reinterpret_cast<const uint32_t*>(&s.tab[i]);
    uint32_t* dst = reinterpret_cast<uint32_t*>(&held);
    for (unsigned k = tid; k < sizeof(DeviceTable) / 4; k += kEncodeThreads) dst[k] = src[k];
    __syncthreads();

    const Game& g = held.g;
    const int P = L.r.players, cur = g.to_move;
    bool on = active ? active[i] != 0 : (flags ? (flags[i] & 0xff) < 2 : true);
    on = on && g.started && consistent(L, g);          // uniform over the workgroup; 0 <= cur < P

    const size_t obs0 = (size_t)i * r.obs_w, share0 = (size_t)i * r.share_w, avail0 = (size_t)i * r.avail_w;
    float* ob = image + r.obs_at + (obs0 & 3);
    float* sh = image + r.share_at + (share0 & 3);
    float* av = image + r.avail_at + (avail0 & 3);
    if (on) {
        // one lane per (view, unit): view 0 is the observation row; then the centralised row's views -- the mover's
        // behind its own hand, or every player's in turn.  Units write disjoint parts of a view, views disjoint rows.
        const int units = view_units(L), views = 1 + (r.share_mode == 0 ? 1 : P);
        for (int w = tid; w < views * units; w += kEncodeThreads) {
            const int view = w / units, unit = w - view * units;
            if (view == 0) encode_view_unit(L, g, cur, unit, ob);
            else if (r.share_mode == 0) encode_view_unit(L, g, cur, unit, sh + L.own_len);
            else encode_view_unit(L, g, view - 1, unit, sh + (size_t)(view - 1) * L.obs_len);
        }
        if (tid < L.num_moves && legal(L, g, move_of(L, tid))) av[tid] = 1.0f;
        if (tid == kEncodeThreads - 1) {               // the one-hot turns, and the mover's own hand
            ob[L.obs_len + cur] = 1.0f;
            if (r.share_mode == 0) {
                encode_own_hand_ones(L, g, cur, sh);
                sh[L.own_len + L.obs_len + cur] = 1.0f;
            } else {
                sh[(size_t)P * L.obs_len + cur] = 1.0f;
            }
        }
    }
    if (tid == 0 && r.to_move) r.to_move[i] = on ? cur : -1;
    __syncthreads();

    stream_row(r.obs, obs0, r.obs_w, image + r.obs_at);
    stream_row(r.share, share0, r.share_w, image + r.share_at);
    stream_row(r.avail, avail0, r.avail_w, image + r.avail_at);
}

// --------------------------------------------------------------------------------------------- host side
int layout_of(int colors, int ranks, int players, int hand_size, int info, int lives, int observation_type,
              int random_start_player, Layout* L) {
    if (random_start_player != 0) return MAPPO_E_SHAPE;      // its uniform_int_distribution differs between libraries
    const hanabi_rules_t rules{colors, ranks, players, hand_size, info, lives, observation_type, 0};
    if (info > 1024 || lives > 1024) return MAPPO_E_SHAPE;
    return make_layout(rules, L) ? kOk : MAPPO_E_SHAPE;
}

int rows_of(const Layout& L, int share_mode, float* obs, float* share, float* avail, int32_t* to_move, Rows* r) {
    if (share_mode != HANABI_SHARE_OWN_HAND && share_mode != HANABI_SHARE_ALL_PLAYERS) return MAPPO_E_SHAPE;
    const int P = L.r.players;
    r->obs = obs, r->share = share, r->avail = avail, r->to_move = to_move;
    r->obs_w = L.obs_len + P;
    r->share_w = (share_mode == HANABI_SHARE_OWN_HAND ? L.own_len + L.obs_len : P * L.obs_len) + P;
    r->avail_w = L.num_moves;
    r->obs_at = 0;
    r->share_at = region_floats(r->obs_w);
    r->avail_at = r->share_at + region_floats(r->share_w);
    r->image_floats = r->avail_at + region_floats(r->avail_w);
    r->share_mode = share_mode;
    if ((size_t)r->image_floats * sizeof(float) > kMaxImageBytes) return MAPPO_E_SHAPE;
    if (L.num_moves > kEncodeThreads) return MAPPO_E_SHAPE;
    if (!mappo::aligned_to(obs, 16) || !mappo::aligned_to(share, 16) || !mappo::aligned_to(avail, 16)) return MAPPO_E_ALIGN;
    return kOk;
}

int check_tables(const void* state, long long n) {
    if (n <= 0 || n > kMaxTables) return MAPPO_E_SHAPE;
    return mappo::aligned_to(state, 4) ? kOk : MAPPO_E_ALIGN;
}

unsigned per_thread_grid(long long n) { return (unsigned)((n + 63) / 64); }

int encode(const State& s, const Layout& L, const Rows& r, const uint8_t* active, const int32_t* flags, hipStream_t st) {
    hipLaunchKernelGGL(hanabi_encode_kernel, dim3((unsigned)s.n), dim3(kEncodeThreads),
                       (size_t)r.image_floats * sizeof(float), st, s, L, r, active, flags);
    return (int)hipGetLastError();
}

}  // namespace

#define HANABI_RULE_PARAMS                                                                                             \
    int32_t colors, int32_t ranks, int32_t players, int32_t hand_size, int32_t max_information_tokens,                 \
        int32_t max_life_tokens, int32_t observation_type, int32_t random_start_player
#define HANABI_RULE_ARGS                                                                                               \
    colors, ranks, players, hand_size, max_information_tokens, max_life_tokens, observation_type, random_start_player

extern "C" int64_t mappo_hanabi_state_bytes(HANABI_RULE_PARAMS) {
    Layout L;
    const int rc = layout_of(HANABI_RULE_ARGS, &L);
    return rc != kOk ? rc : (int64_t)(kMtWords * sizeof(uint32_t) + sizeof(DeviceTable));
}

extern "C" int mappo_hanabi_dims(HANABI_RULE_PARAMS, int32_t* dims) {
    if (!dims) return MAPPO_E_NULL;
    Layout L;
    const int rc = layout_of(HANABI_RULE_ARGS, &L);
    if (rc != kOk) return rc;
    dims[0] = L.r.players, dims[1] = L.num_moves, dims[2] = L.obs_len, dims[3] = L.own_len, dims[4] = L.r.hand_size;
    return kOk;
}

extern "C" int mappo_hanabi_seed(void* state, const int32_t* seeds, int64_t n_tables, mappo_stream_t stream_) {
    if (!state || !seeds) return MAPPO_E_NULL;
    const int rc = check_tables(state, n_tables);
    if (rc != kOk) return rc;
    hipLaunchKernelGGL(hanabi_seed_kernel, dim3(per_thread_grid(n_tables)), dim3(64), 0,
                       static_cast<hipStream_t>(stream_), carve(state, n_tables), seeds);
    return (int)hipGetLastError();
}

extern "C" int mappo_hanabi_reset(void* state, const uint8_t* choose, float* obs, float* share_obs, float* available,
                                  int32_t* to_move, int32_t* flags, int64_t n_tables, int share_mode,
                                  HANABI_RULE_PARAMS, mappo_stream_t stream_) {
    if (!state || !choose || !obs || !share_obs || !available || !flags) return MAPPO_E_NULL;
    Layout L;
    Rows r;
    int rc = layout_of(HANABI_RULE_ARGS, &L);
    if (rc == kOk) rc = check_tables(state, n_tables);
    if (rc == kOk) rc = rows_of(L, share_mode, obs, share_obs, available, to_move, &r);
    if (rc != kOk) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream_);
    const State s = carve(state, n_tables);
    hipLaunchKernelGGL(hanabi_deal_kernel, dim3(per_thread_grid(n_tables)), dim3(64), 0, st, s, L, choose, flags);
    rc = (int)hipGetLastError();
    return rc != 0 ? rc : encode(s, L, r, choose, nullptr, st);
}

extern "C" int mappo_hanabi_step(void* state, const int32_t* actions, float* rewards, uint8_t* status, int32_t* scores,
                                 float* obs, float* share_obs, float* available, int32_t* to_move, int32_t* flags,
                                 int64_t n_tables, int share_mode, HANABI_RULE_PARAMS, mappo_stream_t stream_) {
    if (!state || !actions || !rewards || !status || !scores || !obs || !share_obs || !available || !flags)
        return MAPPO_E_NULL;
    Layout L;
    Rows r;
    int rc = layout_of(HANABI_RULE_ARGS, &L);
    if (rc == kOk) rc = check_tables(state, n_tables);
    if (rc == kOk) rc = rows_of(L, share_mode, obs, share_obs, available, to_move, &r);
    if (rc != kOk) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream_);
    const State s = carve(state, n_tables);
    hipLaunchKernelGGL(hanabi_apply_kernel, dim3(per_thread_grid(n_tables)), dim3(64), 0, st, s, L, actions, rewards,
                       status, scores, flags);
    rc = (int)hipGetLastError();
    return rc != 0 ? rc : encode(s, L, r, nullptr, flags, st);
}

extern "C" int mappo_hanabi_encode(const void* state, const uint8_t* active, float* obs, float* share_obs,
                                   float* available, int32_t* to_move, int64_t n_tables, int share_mode,
                                   HANABI_RULE_PARAMS, mappo_stream_t stream_) {
    if (!state || !obs || !share_obs || !available) return MAPPO_E_NULL;
    Layout L;
    Rows r;
    int rc = layout_of(HANABI_RULE_ARGS, &L);
    if (rc == kOk) rc = check_tables(state, n_tables);
    if (rc == kOk) rc = rows_of(L, share_mode, obs, share_obs, available, to_move, &r);
    if (rc != kOk) return rc;
    return encode(carve(const_cast<void*>(state), n_tables), L, r, active, nullptr, static_cast<hipStream_t>(stream_));
}

extern "C" int mappo_hanabi_draws(const void* state, int32_t* draws, int64_t n_tables, mappo_stream_t stream_) {
    if (!state || !draws) return MAPPO_E_NULL;
    const int rc = check_tables(state, n_tables);
    if (rc != kOk) return rc;
    hipLaunchKernelGGL(hanabi_draws_kernel, dim3(per_thread_grid(n_tables)), dim3(64), 0,
                       static_cast<hipStream_t>(stream_), carve(const_cast<void*>(state), n_tables), draws);
    return (int)hipGetLastError();
}
