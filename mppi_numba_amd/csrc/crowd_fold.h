// crowd_fold.h -- how a tile's wall bits become hits when some of the walls stand for ONE obstacle (a body fleet: the body
// discs of another robot, fleet_kernels.h).  Plain C++ without a HIP type: a host program compiles it on its own
// (tests/test_fleet_body_model.py compares it with a loop over the groups).
//
// mask: bit l is set iff wall l of the tile is hit.  The first g walls of the tile lie in aligned groups of `group`
// (1, 2, 4 or 8: it divides the tile of 64, and g is a multiple of it); a group counts once, however many of its walls
// are hit.  The walls from g on count one each.  group = 1, or g = 0: the population count of the mask.
#pragma once

// the lowest bit of every aligned group
constexpr unsigned long long crowd_fold_leaders(int group) {
  return group >= 8 ? 0x0101010101010101ull : group >= 4 ? 0x1111111111111111ull : group >= 2 ? 0x5555555555555555ull : ~0ull;
}

// log2(group) shift-ORs bring the OR of bits p .. p + group - 1 to bit p; a leader's window is its own group, and the
// bits from g on were masked out before, so the last group takes nothing from the singles behind it.
constexpr int crowd_fold_count(unsigned long long mask, int group, int g) {
  const unsigned long long low = g >= 64 ? ~0ull : g <= 0 ? 0ull : (1ull << g) - 1ull;
  unsigned long long m = mask & low;
  for (int s = 1; s < group; s <<= 1) m |= m >> s;
  return __builtin_popcountll(m & crowd_fold_leaders(group)) + __builtin_popcountll(mask & ~low);
}

// the grouped walls of the tile that starts at wall wbase, when the first `grouped` walls of the set are grouped
constexpr int crowd_fold_span(int grouped, int wbase) {
  return grouped - wbase < 0 ? 0 : grouped - wbase > 64 ? 64 : grouped - wbase;
}

static_assert(crowd_fold_count(0xF0F0ull, 4, 16) == 2 && crowd_fold_count(0xF0F0ull, 1, 0) == 8 && crowd_fold_count(0x1F3ull, 4, 8) == 3 &&
                  crowd_fold_count(~0ull, 8, 64) == 8 && crowd_fold_count(~0ull, 2, 62) == 33 && crowd_fold_span(72, 64) == 8,
              "crowd_fold_count: one hit per aligned group below g, one per bit from g on");
