// Sanitizer driver for dg::Game (CPU only): random legal games with masks, undo and scoring.
// Built and run by tools/sanitize.sh; by hand, from the repository root:
//   g++ -std=c++17 -O1 -g -fno-omit-frame-pointer -fsanitize=address,undefined \
//       csrc/engine/tests/game_main.cpp csrc/engine/go_engine.cpp -o game_main && ./game_main
//
// Checks, beyond "no sanitizer report":
//   * undo after every move restores stones, ages, ko, side to move, ply and key;
//   * in the first six games, which have no voluntary pass: planes() after the last move
//     equals game_positions' row for those moves and one more;
//   * every unmasked point can be played, and never repeats an earlier position;
//   * black area + white area <= 361, and a full undo ends on the empty board.
#include <cstdio>
#include <cstring>
#include <set>
#include <vector>

#include "../go_engine.h"

using namespace dg;

static uint64_t g_rng = 0x2545F4914F6CDD1Dull;
static int g_plane_checks = 0;
static uint32_t rnd(uint32_t n) {
  g_rng ^= g_rng << 13;
  g_rng ^= g_rng >> 7;
  g_rng ^= g_rng << 17;
  return (uint32_t)((g_rng >> 32) % n);
}

#define CHECK(cond)                                                    \
  do {                                                                 \
    if (!(cond)) {                                                     \
      std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
      return 1;                                                        \
    }                                                                  \
  } while (0)

// check_planes: a game without voluntary passes, whose planes() are compared with
// game_positions (which knows no passes) after the last move
static int one_game(int max_moves, bool check_planes) {
  Game g;
  std::vector<Move> moves;
  std::set<uint64_t> seen{g.key()};
  std::vector<uint8_t> mask(NN), pl(NUM_STORED * NN);
  bool any_pass = false;
  for (int m = 0; m < max_moves; ++m) {
    const int player = g.to_move();
    g.legal_mask(player, false, true, rnd(2) != 0, mask.data());
    std::vector<int> ok;
    for (int i = 0; i < NN; ++i)
      if (!mask[i]) ok.push_back(i);
    // the state a move must give back
    const auto stones = g.board().stones(), ages = g.board().ages();
    const int ko = g.ko(), ply = g.ply();
    const uint64_t key = g.key();
    const bool pass = ok.empty() || (!check_planes && rnd(40) == 0);
    int idx = -1;
    if (pass) {
      g.pass_(player);
      CHECK(g.ko() == -1 && g.last_was_pass() && g.key() == key);
    } else {
      idx = ok[rnd((uint32_t)ok.size())];
      g.play(player, idx / N, idx % N);
      CHECK(!seen.count(g.key()));            // positional superko held
      CHECK(g.key() == position_key(g.board().stones()));
    }
    CHECK(g.to_move() == 3 - player && g.ply() == ply + 1);
    CHECK(g.undo());
    CHECK(g.board().stones() == stones && g.board().ages() == ages && g.ko() == ko);
    CHECK(g.to_move() == player && g.ply() == ply && g.key() == key);
    if (pass) {
      g.pass_(player);
      any_pass = true;
    } else {
      g.play(player, idx / N, idx % N);
      moves.push_back({player, idx / N, idx % N});
      seen.insert(g.key());
    }
    int b = 0, w = 0;
    g.score(&b, &w);
    CHECK(b >= 0 && w >= 0 && b + w <= NN);
  }
  if (check_planes && !any_pass) {   // (game_positions knows no passes: ages would differ)
    std::vector<uint8_t> all((moves.size() + 1) * NUM_STORED * NN);
    std::vector<Move> probe = moves;
    int e = 0;                       // a further row: the position after the last move
    while (e < NN && g.board().at(e) != 0) ++e;
    if (e < NN) {
      probe.push_back({g.to_move(), e / N, e % N});
      game_positions({}, probe, all.data(), true);
      g.planes(pl.data(), true);
      CHECK(std::memcmp(pl.data(), all.data() + moves.size() * NUM_STORED * NN,
                        NUM_STORED * NN) == 0);
      ++g_plane_checks;
    }
  }
  while (g.undo()) {
  }
  CHECK(g.ply() == 0 && g.key() == 0 && g.to_move() == 1);
  for (int i = 0; i < NN; ++i) CHECK(g.board().at(i) == 0 && g.board().ages()[i] == 0);
  // an occupied point throws and changes nothing
  g.play(1, 3, 3);
  try {
    g.play(2, 3, 3);
    CHECK(false);
  } catch (const IllegalMove&) {
  }
  CHECK(g.ply() == 1 && g.to_move() == 2);
  return 0;
}

int main() {
  for (int k = 0; k < 12; ++k)
    if (one_game(150 + 60 * k, k < 6)) return 1;
  if (g_plane_checks < 5) {          // (a forced pass, no candidate left, may cost one)
    std::fprintf(stderr, "planes() compared in %d games only\n", g_plane_checks);
    return 1;
  }
  std::printf("game ok (%d plane checks)\n", g_plane_checks);
  return 0;
}
