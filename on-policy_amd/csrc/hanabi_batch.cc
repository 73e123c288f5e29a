// Batched Hanabi stepper: N tables advanced per call, observations written as rows of caller-owned float32 arrays.
// C ABI and the reference file:line of every rule / encoder section: include/hanabi_batch.h.
//
// A table is a fixed-size POD (cards are indices color * ranks + rank, hint knowledge is two bitmasks per hand slot),
// so a batch is one contiguous vector and stepping or encoding it touches no heap.  The only pieces that have to be
// library-identical to the reference engine are the random draws: std::mt19937 + std::discrete_distribution over the
// remaining card counts (hanabi_game.cc:108-114), which is why the host's chance source is C++ <random> itself.  The rules,
// the deal and the encoder sections are hanabi_rules.h, shared with the device stepper (mappo_hanabi.hip).
#include "../../include/hanabi_batch.h"

#include <algorithm>
#include <cstring>
#include <new>
#include <random>
#include <thread>
#include <vector>

#include "hanabi_rules.h"

using namespace hanabi;

namespace {

struct Table {
  std::mt19937 rng;
  Game g;
};

struct StdChance {       // the host's chance source: <random> itself
  std::mt19937 &rng;
  int pick(const double *w, int n) {
    std::discrete_distribution<std::mt19937::result_type> d(w, w + n);
    return (int)d(rng);
  }
  int first_player(int players) {
    std::uniform_int_distribution<std::mt19937::result_type> first(0, players - 1);
    return (int)first(rng);
  }
};

}  // namespace

struct hanabi_batch {
  Layout L;
  std::vector<Table> tables;
  int failed_table;
};

namespace {

template <typename T>
void encode_view(const Layout &L, const Game &t, int observer, T *out) {
  std::fill(out, out + L.obs_len, T(0));
  encode_view_ones(L, t, observer, out);
}

template <typename T>
void encode_own_hand(const Layout &L, const Game &t, int observer, T *out) {
  std::fill(out, out + L.own_len, T(0));
  encode_own_hand_ones(L, t, observer, out);
}

// Tables are independent: big batches are split over a few host threads (joined before the call returns).
template <typename F>
void for_each_table(int n, int min_per_thread, F fn) {
  unsigned hw = std::thread::hardware_concurrency();
  int workers = std::min<int>({(int)(hw ? hw : 1), 16, n / min_per_thread});
  if (workers <= 1) {
    for (int i = 0; i < n; ++i) fn(i);
    return;
  }
  std::vector<std::thread> pool;
  pool.reserve(workers - 1);
  auto span = [&](int w) {
    const int lo = (int)((long long)n * w / workers), hi = (int)((long long)n * (w + 1) / workers);
    for (int i = lo; i < hi; ++i) fn(i);
  };
  for (int w = 1; w < workers; ++w) pool.emplace_back(span, w);
  span(0);
  for (auto &th : pool) th.join();
}

}  // namespace

// ------------------------------------------------------------------------------------------------ C ABI
extern "C" {

hanabi_batch_t *hanabi_batch_create(const hanabi_rules_t *rules, int32_t n_tables, const int32_t *seeds) {
  if (!rules || !seeds || n_tables <= 0) return nullptr;
  hanabi_batch *b = new (std::nothrow) hanabi_batch;
  if (!b) return nullptr;
  if (!make_layout(*rules, &b->L)) {
    delete b;
    return nullptr;
  }
  b->failed_table = -1;
  b->tables.resize((size_t)n_tables);
  for (int i = 0; i < n_tables; ++i) {
    b->tables[i].rng.seed(seeds[i]);      // std::mt19937::seed(int) as HanabiGame does (hanabi_game.cc:50)
    b->tables[i].g.started = false;
  }
  return b;
}

void hanabi_batch_destroy(hanabi_batch_t *b) { delete b; }

int32_t hanabi_batch_tables(const hanabi_batch_t *b) { return b ? (int32_t)b->tables.size() : HANABI_BAD_ARGUMENT; }
int32_t hanabi_batch_players(const hanabi_batch_t *b) { return b ? b->L.r.players : HANABI_BAD_ARGUMENT; }
int32_t hanabi_batch_num_moves(const hanabi_batch_t *b) { return b ? b->L.num_moves : HANABI_BAD_ARGUMENT; }
int32_t hanabi_batch_obs_len(const hanabi_batch_t *b) { return b ? b->L.obs_len : HANABI_BAD_ARGUMENT; }
int32_t hanabi_batch_own_hand_len(const hanabi_batch_t *b) { return b ? b->L.own_len : HANABI_BAD_ARGUMENT; }
int32_t hanabi_batch_failed_table(const hanabi_batch_t *b) { return b ? b->failed_table : HANABI_BAD_ARGUMENT; }

int hanabi_batch_reset(hanabi_batch_t *b, const uint8_t *choose) {
  if (!b) return HANABI_BAD_ARGUMENT;
  const int n = (int)b->tables.size();
  for (int i = 0; i < n; ++i)
    if (!choose || choose[i]) {
      StdChance chance{b->tables[i].rng};
      new_game(b->L, &b->tables[i].g, chance);
    }
  return HANABI_OK;
}

int hanabi_batch_step(hanabi_batch_t *b, const int32_t *actions, float *rewards, uint8_t *status, int32_t *scores) {
  if (!b || !actions || !rewards || !status || !scores) return HANABI_BAD_ARGUMENT;
  const Layout &L = b->L;
  const int n = (int)b->tables.size();
  for (int i = 0; i < n; ++i) {
    if (!b->tables[i].g.started) return HANABI_NOT_STARTED;
    if (actions[i] == -1) continue;
    if (!legal(L, b->tables[i].g, move_of(L, actions[i]))) {
      b->failed_table = i;
      return HANABI_ILLEGAL_MOVE;
    }
  }
  for_each_table(n, 2048, [&](int i) {
    Game &t = b->tables[i].g;
    if (actions[i] == -1) {
      rewards[i] = 0.0f;
      status[i] = 2;
      scores[i] = score_of(L, t);
      return;
    }
    const int before = score_of(L, t);
    StdChance chance{b->tables[i].rng};
    apply(L, &t, move_of(L, actions[i]), chance);
    scores[i] = score_of(L, t);
    rewards[i] = (float)(scores[i] - before);
    status[i] = end_of(L, t) != kRunning ? 1 : 0;
  });
  return HANABI_OK;
}

int hanabi_batch_encode(const hanabi_batch_t *b, int share_mode, const uint8_t *active, float *obs, float *share_obs,
                        float *available, int32_t *to_move) {
  if (!b || !obs || !share_obs || !available ||
      (share_mode != HANABI_SHARE_OWN_HAND && share_mode != HANABI_SHARE_ALL_PLAYERS))
    return HANABI_BAD_ARGUMENT;
  const Layout &L = b->L;
  const int n = (int)b->tables.size(), P = L.r.players;
  const size_t obs_w = (size_t)L.obs_len + P;
  const size_t share_w = (size_t)(share_mode == HANABI_SHARE_OWN_HAND ? L.own_len + L.obs_len : P * L.obs_len) + P;
  for (int i = 0; i < n; ++i)
    if ((!active || active[i]) && !b->tables[i].g.started) return HANABI_NOT_STARTED;
  for_each_table(n, 128, [&](int i) {
    float *ob = obs + (size_t)i * obs_w, *sh = share_obs + (size_t)i * share_w, *av = available + (size_t)i * L.num_moves;
    if (active && !active[i]) {
      std::fill(ob, ob + obs_w, 0.0f);
      std::fill(sh, sh + share_w, 0.0f);
      std::fill(av, av + L.num_moves, 0.0f);
      if (to_move) to_move[i] = -1;
      return;
    }
    const Game &t = b->tables[i].g;
    const int cur = t.to_move;
    encode_view(L, t, cur, ob);
    float *turn = ob + L.obs_len;
    for (int p = 0; p < P; ++p) turn[p] = p == cur ? 1.0f : 0.0f;
    if (share_mode == HANABI_SHARE_OWN_HAND) {
      encode_own_hand(L, t, cur, sh);
      std::memcpy(sh + L.own_len, ob, obs_w * sizeof(float));           // observation | turn
    } else {
      for (int p = 0; p < P; ++p) {
        if (p == cur) std::memcpy(sh + (size_t)p * L.obs_len, ob, (size_t)L.obs_len * sizeof(float));
        else encode_view(L, t, p, sh + (size_t)p * L.obs_len);
      }
      std::memcpy(sh + (size_t)P * L.obs_len, turn, (size_t)P * sizeof(float));
    }
    for (int u = 0; u < L.num_moves; ++u) av[u] = legal(L, t, move_of(L, u)) ? 1.0f : 0.0f;
    if (to_move) to_move[i] = cur;
  });
  return HANABI_OK;
}

int hanabi_batch_player_view(const hanabi_batch_t *b, int32_t table, int32_t player, int32_t *obs, int32_t *own_hand) {
  if (!b || table < 0 || table >= (int)b->tables.size() || player < 0 || player >= b->L.r.players)
    return HANABI_BAD_ARGUMENT;
  const Game &t = b->tables[table].g;
  if (!t.started) return HANABI_NOT_STARTED;
  if (obs) encode_view(b->L, t, player, obs);
  if (own_hand) encode_own_hand(b->L, t, player, own_hand);
  return HANABI_OK;
}

int hanabi_batch_table_state(const hanabi_batch_t *b, int32_t table, int32_t *out) {
  if (!b || !out || table < 0 || table >= (int)b->tables.size()) return HANABI_BAD_ARGUMENT;
  const Game &t = b->tables[table].g;
  if (!t.started) return HANABI_NOT_STARTED;
  out[0] = t.lives;
  out[1] = t.info;
  out[2] = t.stock_total;
  out[3] = score_of(b->L, t);
  out[4] = t.to_move;
  out[5] = end_of(b->L, t);
  out[6] = t.turns_left;
  out[7] = t.discards;
  for (int c = 0; c < b->L.r.colors; ++c) out[8 + c] = t.fireworks[c];
  return HANABI_OK;
}

}  // extern "C"
