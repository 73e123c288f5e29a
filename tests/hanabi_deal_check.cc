// Stand-alone check of the device stepper's chance source (csrc/hanabi_rules.h: Mt19937Strided + pick_discrete) against
// what the host stepper and the reference engine draw with: std::mt19937 + std::discrete_distribution.
// Built and run by tests/test_hanabi_deal_cpu.py (g++ -fsanitize=address,undefined).  Prints one line of totals.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../on-policy_amd/csrc/hanabi_rules.h"

int main(int argc, char **argv) {
  const int draws = argc > 1 ? std::atoi(argv[1]) : 20000;
  const size_t stride = 3, column = 1;             // the generator's words lie `stride` apart, as in a batch of 3 tables
  const uint32_t guard = 0xdeadbeefu;
  long long total = 0, mismatches = 0, desynced = 0, trampled = 0;
  uint32_t min_refills = ~0u;
  int seeds = 0, single_weight_draws = 0;
  for (int seed = -3; seed <= 39; ++seed, ++seeds) {
    std::mt19937 ref;
    ref.seed(seed);                                // as HanabiGame does (hanabi_game.cc:50)
    std::vector<uint32_t> words(624 * stride, guard);
    uint32_t idx = 0, drawn = 0;
    hanabi::mt_seed(words.data() + column, stride, (uint32_t)seed, &idx, &drawn);
    hanabi::Mt19937Strided gen{words.data() + column, stride, &idx, &drawn};
    uint32_t lcg = 12345u + (uint32_t)seed * 2654435761u;
    auto next = [&lcg]() { return (lcg = lcg * 1664525u + 1013904223u) >> 8; };
    for (int d = 0; d < draws; ++d, ++total) {
      const int n = 1 + (int)(next() % 25u);       // 1 .. 25 card types still in stock
      int count[hanabi::kMaxCardTypes], sum = 0;
      for (int i = 0; i < n; ++i) sum += count[i] = 1 + (int)(next() % 3u);
      double w[hanabi::kMaxCardTypes];
      for (int i = 0; i < n; ++i) w[i] = static_cast<double>(count[i]) / static_cast<double>(sum);
      const uint32_t before = drawn;
      std::discrete_distribution<std::mt19937::result_type> pick(w, w + n);
      const int expect = (int)pick(ref), got = hanabi::pick_discrete(w, n, gen);
      mismatches += expect != got;
      if (n == 1) {
        ++single_weight_draws;
        mismatches += drawn != before;             // one weight: no random number is consumed
      } else {
        mismatches += drawn != before + 2;
      }
    }
    desynced += (uint32_t)ref() != gen();          // the two generators stand at the same word
    for (size_t k = 0; k < words.size(); ++k)
      if (k % stride != column && words[k] != guard) ++trampled;
    if (drawn / 624u < min_refills) min_refills = drawn / 624u;
  }
  std::printf("seeds=%d draws=%lld mismatches=%lld desynced=%lld trampled=%lld min_refills=%u single=%d\n", seeds, total,
              mismatches, desynced, trampled, min_refills, single_weight_draws);
  return mismatches || desynced || trampled ? 1 : 0;
}
