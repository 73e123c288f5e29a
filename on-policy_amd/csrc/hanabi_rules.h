// The one copy of the Hanabi rules, the deal and the observation encoder: included by the host stepper
// (hanabi_batch.cc -> libhanabi_batch.so, g++) and by the device stepper (mappo_hanabi.hip -> libmappo_hip.so, hipcc).
// Reference file:line of every rule / encoder section: include/hanabi_batch.h.
//
// A game is a fixed-size POD (cards are indices color * ranks + rank, hint knowledge is two bitmasks per hand slot).
// The only pieces that have to be library-identical to the reference engine are the random draws: std::mt19937 +
// std::discrete_distribution over the remaining card counts (hanabi_game.cc:108-114).  The deal is a template on its
// chance source: the host passes <random> itself, the device the hand-written form below (Mt19937Strided +
// pick_discrete), which tests/test_hanabi_deal_cpu.py holds against <random> draw for draw.
#ifndef HANABI_RULES_H_
#define HANABI_RULES_H_

#include <stddef.h>
#include <stdint.h>

#include "../../include/hanabi_batch.h"

#if defined(__HIPCC__)
#define HANABI_HD __host__ __device__
#else
#define HANABI_HD
#endif

namespace hanabi {

constexpr int kMaxColors = 5, kMaxRanks = 5, kMaxPlayers = 5, kMaxHand = 5;
constexpr int kMaxCardTypes = kMaxColors * kMaxRanks;

enum MoveKind : int8_t { kNone = 0, kPlay, kDiscard, kHintColor, kHintRank };
enum EndOfGame { kRunning = 0, kOutOfLives, kOutOfCards, kCompleted };

struct Move {
  MoveKind kind;
  int8_t slot;     // play / discard: position in the hand
  int8_t offset;   // hints: target player relative to the mover (1 .. players - 1)
  int8_t value;    // hints: color or rank
};

struct Layout {    // everything derived from the rules once
  hanabi_rules_t r;
  int card_types, deck_total, num_moves;
  int copies[kMaxRanks];
  int hands_len, board_len, discard_len, last_len, belief_len, obs_len, own_len;
  int deck_bits;
};

struct Slot {
  uint8_t card;          // color * ranks + rank
  uint8_t colors_left;   // bit c set: no hint has ruled color c out
  uint8_t ranks_left;
  int8_t color_hint;     // -1 until a hint named this card's color
  int8_t rank_hint;
};

struct LastMove {        // the most recent player move, as the encoder's last-action section needs it
  MoveKind kind;
  int8_t player, slot, offset, value, card;
  uint8_t touched;       // hints: bit i = slot i matched
  bool scored, regained_token;
};

struct Game {            // one table without its generator
  uint8_t stock[kMaxCardTypes];
  int stock_total;
  Slot hand[kMaxPlayers][kMaxHand];
  uint8_t hand_n[kMaxPlayers];
  uint8_t fireworks[kMaxColors];
  uint8_t discarded[kMaxCardTypes];
  int discards;
  int info, lives;
  int to_move;           // -1 while a card is owed to some hand (chance node)
  int next_player;
  int turns_left;
  LastMove last;
  bool started;
};

HANABI_HD inline bool make_layout(const hanabi_rules_t &in, Layout *L) {
  hanabi_rules_t r = in;
  if (r.players < 2 || r.players > kMaxPlayers || r.colors < 1 || r.colors > kMaxColors || r.ranks < 1 ||
      r.ranks > kMaxRanks || r.max_information_tokens < 0 || r.max_life_tokens < 1 || r.observation_type < 0 ||
      r.observation_type > 2)
    return false;
  if (r.hand_size <= 0) r.hand_size = r.players < 4 ? 5 : 4;
  if (r.hand_size > kMaxHand) return false;
  L->r = r;
  L->card_types = r.colors * r.ranks;
  int per_color = 0;
  for (int k = 0; k < kMaxRanks; ++k) L->copies[k] = 0;
  for (int k = 0; k < r.ranks; ++k) {   // hanabi_game.cc:139-148: three of the lowest rank, one of the highest, else two
    L->copies[k] = k == 0 ? 3 : (k == r.ranks - 1 ? 1 : 2);
    per_color += L->copies[k];
  }
  L->deck_total = per_color * r.colors;
  if (r.hand_size * r.players > L->deck_total) return false;
  L->num_moves = 2 * r.hand_size + (r.players - 1) * (r.colors + r.ranks);
  L->deck_bits = L->deck_total - r.players * r.hand_size;
  L->hands_len = (r.players - 1) * r.hand_size * L->card_types + r.players;
  L->board_len = L->deck_bits + L->card_types + r.max_information_tokens + r.max_life_tokens;
  L->discard_len = L->deck_total;
  L->last_len = r.players + 4 + r.players + r.colors + r.ranks + 2 * r.hand_size + L->card_types + 2;
  L->belief_len = r.observation_type == 0 ? 0 : r.players * r.hand_size * (L->card_types + r.colors + r.ranks);
  L->obs_len = L->hands_len + L->board_len + L->discard_len + L->last_len + L->belief_len;
  L->own_len = r.hand_size * L->card_types;
  return true;
}

HANABI_HD inline Move move_of(const Layout &L, int uid) {
  const int h = L.r.hand_size;
  if (uid < 0 || uid >= L.num_moves) return {kNone, -1, -1, -1};
  if (uid < h) return {kDiscard, (int8_t)uid, -1, -1};
  uid -= h;
  if (uid < h) return {kPlay, (int8_t)uid, -1, -1};
  uid -= h;
  const int color_hints = (L.r.players - 1) * L.r.colors;
  if (uid < color_hints) return {kHintColor, -1, (int8_t)(1 + uid / L.r.colors), (int8_t)(uid % L.r.colors)};
  uid -= color_hints;
  return {kHintRank, -1, (int8_t)(1 + uid / L.r.ranks), (int8_t)(uid % L.r.ranks)};
}

HANABI_HD inline int score_of(const Layout &L, const Game &t) {
  if (t.lives <= 0) return 0;
  int s = 0;
  for (int c = 0; c < L.r.colors; ++c) s += t.fireworks[c];
  return s;
}

HANABI_HD inline EndOfGame end_of(const Layout &L, const Game &t) {
  if (t.lives < 1) return kOutOfLives;
  if (score_of(L, t) >= L.card_types) return kCompleted;
  if (t.turns_left <= 0) return kOutOfCards;
  return kRunning;
}

HANABI_HD inline int hand_owed_a_card(const Layout &L, const Game &t) {
  for (int p = 0; p < L.r.players; ++p)
    if (t.hand_n[p] < L.r.hand_size) return p;
  return -1;
}

HANABI_HD inline void pass_turn(const Layout &L, Game *t) {
  if (t->stock_total > 0 && hand_owed_a_card(L, *t) >= 0) {
    t->to_move = -1;
  } else {
    t->to_move = t->next_player;
    t->next_player = (t->to_move + 1) % L.r.players;
  }
}

HANABI_HD inline bool legal(const Layout &L, const Game &t, const Move &m) {
  if (t.to_move < 0) return false;
  switch (m.kind) {
    case kDiscard:
      return t.info < L.r.max_information_tokens && m.slot < t.hand_n[t.to_move];
    case kPlay:
      return m.slot < t.hand_n[t.to_move];
    case kHintColor:
    case kHintRank: {
      if (t.info <= 0 || m.offset < 1 || m.offset >= L.r.players) return false;
      const int target = (t.to_move + m.offset) % L.r.players;
      for (int i = 0; i < t.hand_n[target]; ++i) {
        const int card = t.hand[target][i].card;
        if ((m.kind == kHintColor ? card / L.r.ranks : card % L.r.ranks) == m.value) return true;
      }
      return false;
    }
    default:
      return false;
  }
}

// Every count and index of a started game is inside what the rules allow -- what the encoder and apply() rely on for
// their own bounds.  The device stepper asks before it trusts state memory it did not just write.
HANABI_HD inline bool consistent(const Layout &L, const Game &t) {
  const hanabi_rules_t &r = L.r;
  if (t.stock_total < 0 || t.stock_total > L.deck_bits || t.info < 0 || t.info > r.max_information_tokens ||
      t.lives < 0 || t.lives > r.max_life_tokens || t.to_move < 0 || t.to_move >= r.players || t.next_player < 0 ||
      t.next_player >= r.players)
    return false;
  for (int p = 0; p < r.players; ++p) {
    if (t.hand_n[p] > r.hand_size) return false;
    for (int i = 0; i < t.hand_n[p]; ++i) {
      const Slot &s = t.hand[p][i];
      if (s.card >= L.card_types || s.color_hint >= r.colors || s.rank_hint >= r.ranks) return false;
    }
  }
  for (int c = 0; c < r.colors; ++c)
    if (t.fireworks[c] > r.ranks) return false;
  for (int k = 0; k < L.card_types; ++k)
    if (t.discarded[k] > L.copies[k % r.ranks] || t.stock[k] > L.copies[k % r.ranks]) return false;
  const LastMove &m = t.last;
  if (m.kind < kNone || m.kind > kHintRank) return false;
  if (m.kind == kNone) return true;
  if (m.player < 0 || m.player >= r.players) return false;
  if (m.kind == kPlay || m.kind == kDiscard)
    return m.slot >= 0 && m.slot < r.hand_size && m.card >= 0 && m.card < L.card_types;
  return m.offset >= 1 && m.offset < r.players && m.value >= 0 && m.value < (m.kind == kHintColor ? r.colors : r.ranks);
}

// ------------------------------------------------------------------------------------------- chance
// std::mt19937 with its 624 words `stride` apart (word k of a table at s[k * stride]): a batch keeps them as [624][N], so
// the tables of a wave read and write neighbouring addresses.  A word is regenerated in place when it is next due
// (word i from i, i + 1 and i + 397, the standard recurrence); that gives the very sequence of the library's
// 624-at-a-time refill, which reads exactly these operands in this order.  *idx is the next word (624 after seeding, as
// the library sets it; it wraps to 0), *drawn counts the 32-bit words taken.
struct Mt19937Strided {
  uint32_t *s;
  size_t stride;
  uint32_t *idx, *drawn;

  HANABI_HD uint32_t operator()() {
    uint32_t i = *idx;
    if (i >= 624u) i = 0;
    const uint32_t i1 = i + 1 == 624u ? 0 : i + 1, im = i + 397 >= 624u ? i + 397 - 624u : i + 397;
    const uint32_t y = (s[i * stride] & 0x80000000u) | (s[i1 * stride] & 0x7fffffffu);
    uint32_t v = s[im * stride] ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
    s[i * stride] = v;
    *idx = i + 1;
    ++*drawn;
    v ^= v >> 11;
    v ^= (v << 7) & 0x9d2c5680u;
    v ^= (v << 15) & 0xefc60000u;
    v ^= v >> 18;
    return v;
  }
};

// std::mt19937::seed(value): value taken modulo 2^32 (an int32 seed converts that way).
HANABI_HD inline void mt_seed(uint32_t *s, size_t stride, uint32_t seed, uint32_t *idx, uint32_t *drawn) {
  uint32_t prev = seed;
  s[0] = prev;
  for (uint32_t k = 1; k < 624u; ++k) {
    prev = 1812433253u * (prev ^ (prev >> 30)) + k;
    s[k * stride] = prev;
  }
  *idx = 624u;
  *drawn = 0;
}

// std::discrete_distribution<>(w, w + n)(gen) of libstdc++, written out: normalise by the sum, running sums with the
// last one set to 1, p = generate_canonical<double, 53> from two 32-bit outputs (low word first; the addition rounds,
// and that rounding is part of the rule), the first running sum >= p.  One weight: no random number is consumed.
// Must be compiled without floating-point contraction.
template <class Gen>
HANABI_HD inline int pick_discrete(const double *w, int n, Gen &gen) {
  if (n < 2) return 0;
  if (n > kMaxCardTypes) n = kMaxCardTypes;
  double sum = 0.0;
  for (int i = 0; i < n; ++i) sum += w[i];
  double cp[kMaxCardTypes];
  double run = 0.0;
  for (int i = 0; i < n; ++i) {
    run += w[i] / sum;
    cp[i] = run;
  }
  cp[n - 1] = 1.0;
  const double lo = (double)gen(), hi = (double)gen();
  double p = (lo + hi * 4294967296.0) / 18446744073709551616.0;
  if (p >= 1.0) p = 0x1.fffffffffffffp-1;              // the largest double below 1
  int k = 0;
  while (k < n - 1 && cp[k] < p) ++k;
  return k;
}

struct MtChance {        // the device's chance source
  Mt19937Strided gen;
  HANABI_HD int pick(const double *w, int n) { return pick_discrete(w, n, gen); }
  HANABI_HD int first_player(int) { return 0; }        // random_start_player is refused before a kernel runs
};

// One card from the stock to the first short hand.  The draw is the reference's: a discrete distribution over the
// card types still in stock, weights count / stock size, in card-index order (hanabi_state.cc:327-339 +
// hanabi_game.cc:108-114).  (With one type left the distribution consumes no random number -- same class, same rule.)
template <class Chance>
HANABI_HD inline void deal_one(const Layout &L, Game *t, Chance &chance) {
  double weight[kMaxCardTypes];
  int type_of[kMaxCardTypes];
  int n = 0;
  for (int i = 0; i < L.card_types; ++i) {
    if (t->stock[i] > 0) {
      weight[n] = static_cast<double>(t->stock[i]) / static_cast<double>(t->stock_total);
      type_of[n++] = i;
    }
  }
  const int p = hand_owed_a_card(L, *t);
  if (n == 0 || p < 0) {                  // nothing to deal (never the case in a consistent game): the turn passes
    t->stock_total = 0;
    pass_turn(L, t);
    return;
  }
  const int card = type_of[chance.pick(weight, n)];
  --t->stock[card];
  --t->stock_total;
  Slot &s = t->hand[p][t->hand_n[p]++];
  s.card = (uint8_t)card;
  s.colors_left = (uint8_t)((1u << L.r.colors) - 1);
  s.ranks_left = (uint8_t)((1u << L.r.ranks) - 1);
  s.color_hint = s.rank_hint = -1;
  if (L.r.observation_type == 2) {      // seer: dealt cards are known outright (hanabi_state.cc:230-233)
    s.color_hint = (int8_t)(card / L.r.ranks);
    s.rank_hint = (int8_t)(card % L.r.ranks);
    s.colors_left = (uint8_t)(1u << s.color_hint);
    s.ranks_left = (uint8_t)(1u << s.rank_hint);
  }
  pass_turn(L, t);
}

// Cards until a player is to move: a whole deal is players * hand_size cards, a move owes at most one.
template <class Chance>
HANABI_HD inline void deal_until_a_player_moves(const Layout &L, Game *t, Chance &chance) {
  for (int k = 0; k < L.r.players * L.r.hand_size && t->to_move < 0; ++k) deal_one(L, t, chance);
}

template <class Chance>
HANABI_HD inline void new_game(const Layout &L, Game *t, Chance &chance) {
  for (int i = 0; i < kMaxCardTypes; ++i) {
    t->stock[i] = i < L.card_types ? (uint8_t)L.copies[i % L.r.ranks] : 0;
    t->discarded[i] = 0;
  }
  t->stock_total = L.deck_total;
  for (int p = 0; p < kMaxPlayers; ++p) t->hand_n[p] = 0;
  for (int c = 0; c < kMaxColors; ++c) t->fireworks[c] = 0;
  t->discards = 0;
  t->info = L.r.max_information_tokens;
  t->lives = L.r.max_life_tokens;
  t->to_move = -1;
  t->next_player = 0;
  if (L.r.random_start_player) t->next_player = chance.first_player(L.r.players);      // hanabi_game.cc:150-157
  t->turns_left = L.r.players;
  t->last = LastMove{kNone, -1, -1, -1, -1, -1, 0, false, false};
  t->started = true;
  deal_until_a_player_moves(L, t, chance);
}

HANABI_HD inline void remove_slot(Game *t, int p, int slot) {
  for (int i = slot; i + 1 < t->hand_n[p]; ++i) t->hand[p][i] = t->hand[p][i + 1];
  --t->hand_n[p];
}

// `m` must be legal(L, *t, m).
template <class Chance>
HANABI_HD inline void apply(const Layout &L, Game *t, const Move &m, Chance &chance) {
  if (t->stock_total == 0) --t->turns_left;          // hanabi_state.cc:220-222
  const int p = t->to_move;
  LastMove last{m.kind, (int8_t)p, m.slot, m.offset, m.value, -1, 0, false, false};
  switch (m.kind) {
    case kDiscard: {
      if (t->info < L.r.max_information_tokens) {
        ++t->info;
        last.regained_token = true;
      }
      const int card = t->hand[p][m.slot].card;
      last.card = (int8_t)card;
      ++t->discarded[card];
      ++t->discards;
      remove_slot(t, p, m.slot);
      break;
    }
    case kPlay: {
      const int card = t->hand[p][m.slot].card;
      const int color = card / L.r.ranks, rank = card % L.r.ranks;
      last.card = (int8_t)card;
      if (rank == t->fireworks[color]) {
        last.scored = true;
        if (++t->fireworks[color] == L.r.ranks && t->info < L.r.max_information_tokens) {
          ++t->info;                                   // finished stack hands a token back
          last.regained_token = true;
        }
      } else {
        --t->lives;
        ++t->discarded[card];
        ++t->discards;
      }
      remove_slot(t, p, m.slot);
      break;
    }
    case kHintColor:
    case kHintRank: {
      --t->info;
      const int target = (p + m.offset) % L.r.players;
      for (int i = 0; i < t->hand_n[target]; ++i) {
        Slot &s = t->hand[target][i];
        if (m.kind == kHintColor) {
          if (s.card / L.r.ranks == m.value) {
            last.touched |= (uint8_t)(1u << i);
            s.color_hint = m.value;
            s.colors_left = (uint8_t)(1u << m.value);
          } else {
            s.colors_left &= (uint8_t)~(1u << m.value);
          }
        } else {
          if (s.card % L.r.ranks == m.value) {
            last.touched |= (uint8_t)(1u << i);
            s.rank_hint = m.value;
            s.ranks_left = (uint8_t)(1u << m.value);
          } else {
            s.ranks_left &= (uint8_t)~(1u << m.value);
          }
        }
      }
      break;
    }
    default:
      break;
  }
  t->last = last;
  pass_turn(L, t);
  deal_until_a_player_moves(L, t, chance);
}

// ---------------------------------------------------------------------------------------------- encoder
// A view (one observer's row of L.obs_len entries) is encoded in independent UNITS that write disjoint parts of it: one
// per other player's hand, the "hand is short" bits, the board, the discards, the last move, and one per hand slot of the
// card-knowledge section.  The host runs them in order (encode_view_ones); the device gives every unit of every view of
// a table its own lane.  A unit sets the ones of an all-zero row (the caller clears it), so the same code fills float
// rows (batched paths) and int vectors (player_view).
HANABI_HD inline int view_units(const Layout &L) {
  return L.r.players + 3 + (L.belief_len ? L.r.players * L.r.hand_size : 0);
}

template <typename T>
HANABI_HD inline void encode_view_unit(const Layout &L, const Game &t, int observer, int unit, T *out) {
  const hanabi_rules_t &r = L.r;
  const int P = r.players, H = r.hand_size, K = L.card_types;
  if (unit < 0) return;
  if (unit < P - 1) {            // one other player's cards, observer-relative order
    const int off = unit + 1, p = (observer + off) % P;
    T *o = out + (off - 1) * H * K;
    for (int i = 0; i < t.hand_n[p]; ++i) o[i * K + t.hand[p][i].card] = T(1);
    return;
  }
  if (unit == P - 1) {           // one "hand is short" bit per player
    T *o = out + (P - 1) * H * K;
    for (int off = 0; off < P; ++off)
      if (t.hand_n[(observer + off) % P] < H) o[off] = T(1);
    return;
  }
  if (unit == P) {               // board: deck thermometer, fireworks one-hot (highest rank played), token thermometers
    T *o = out + L.hands_len;
    for (int i = 0; i < t.stock_total; ++i) o[i] = T(1);
    o += L.deck_bits;
    for (int c = 0; c < r.colors; ++c) {
      if (t.fireworks[c] > 0) o[t.fireworks[c] - 1] = T(1);
      o += r.ranks;
    }
    for (int i = 0; i < t.info; ++i) o[i] = T(1);
    o += r.max_information_tokens;
    for (int i = 0; i < t.lives; ++i) o[i] = T(1);
    return;
  }
  if (unit == P + 1) {           // discards: thermometer per card type, as many bits as the type has copies
    T *o = out + L.hands_len + L.board_len;
    for (int k = 0; k < K; ++k) {
      for (int i = 0; i < t.discarded[k]; ++i) o[i] = T(1);
      o += L.copies[k % r.ranks];
    }
    return;
  }
  if (unit == P + 2) {           // last player move
    if (t.last.kind == kNone) return;
    const LastMove &m = t.last;
    const int who = (m.player - observer + P) % P;
    T *q = out + L.hands_len + L.board_len + L.discard_len;
    q[who] = T(1);
    q += P;
    q[m.kind == kPlay ? 0 : m.kind == kDiscard ? 1 : m.kind == kHintColor ? 2 : 3] = T(1);
    q += 4;
    const bool hint = m.kind == kHintColor || m.kind == kHintRank;
    if (hint) q[(who + m.offset) % P] = T(1);
    q += P;
    if (m.kind == kHintColor) q[m.value] = T(1);
    q += r.colors;
    if (m.kind == kHintRank) q[m.value] = T(1);
    q += r.ranks;
    if (hint)
      for (int i = 0; i < H; ++i)
        if (m.touched & (1u << i)) q[i] = T(1);
    q += H;
    if (!hint) q[m.slot] = T(1);
    q += H;
    if (!hint) q[m.card] = T(1);
    q += K;
    if (m.kind == kPlay) {
      if (m.scored) q[0] = T(1);
      if (m.regained_token) q[1] = T(1);
    }
    return;
  }
  // card knowledge of one hand slot (observer's hand first).  The reference weights the possible-card bits by how many
  // copies are neither discarded nor on the fireworks, then divides by the row total IN INTEGERS
  // (canonical_encoders.cc:509-530): what survives is a 1 where exactly one card type is still possible, 0 elsewhere.
  const int slot_unit = unit - (P + 3);
  if (!L.belief_len || slot_unit >= P * H) return;
  const int off = slot_unit / H, i = slot_unit % H, p = (observer + off) % P;
  if (i >= t.hand_n[p]) return;
  const int per_slot = K + r.colors + r.ranks;
  const Slot &s = t.hand[p][i];
  T *q = out + L.hands_len + L.board_len + L.discard_len + L.last_len + (off * H + i) * per_slot;
  // (int)(w_k / sum w) is 1 exactly when w_k is the only non-zero weight (all values are small integers, exact in
  // float), so the division is a count of the card types that are possible AND still unaccounted for
  int candidates = 0, only = -1;
  for (int k = 0; k < K; ++k) {
    const int color = k / r.ranks, rank = k % r.ranks;
    const int remaining = L.copies[rank] - t.discarded[k] - (rank < t.fireworks[color] ? 1 : 0);
    if (remaining > 0 && ((s.colors_left >> color) & 1) && ((s.ranks_left >> rank) & 1)) {
      ++candidates;
      only = k;
    }
  }
  if (candidates == 1) q[only] = T(1);
  if (s.color_hint >= 0) q[K + s.color_hint] = T(1);
  if (s.rank_hint >= 0) q[K + r.colors + s.rank_hint] = T(1);
}

template <typename T>
HANABI_HD inline void encode_view_ones(const Layout &L, const Game &t, int observer, T *out) {
  for (int unit = 0, n = view_units(L); unit < n; ++unit) encode_view_unit(L, t, observer, unit, out);
}

template <typename T>
HANABI_HD inline void encode_own_hand_ones(const Layout &L, const Game &t, int observer, T *out) {
  for (int i = 0; i < t.hand_n[observer]; ++i) out[i * L.card_types + t.hand[observer][i].card] = T(1);
}

}  // namespace hanabi
#endif  // HANABI_RULES_H_
