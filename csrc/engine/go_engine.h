// Go rules engine + tactical feature extractor (CPU, C++17).
//
// Semantics follow the reference's Lua engine exactly (makedata.lua), so the stored
// planes it produces match the bundled fixture bit for bit:
//   * trial play (play_with_f, makedata.lua:388-391 / apply_f_to_dead_neighbors :234-241):
//     place the stone, clear every adjacent opponent group left with 0 liberties (in the
//     neighbour order up, down, left, right), then clear the player's own group if it has
//     0 liberties (suicide is legal and removes own stones).  Ko is not enforced.
//   * simple ko (an addition, off by default): a move that captures exactly one stone with
//     a lone stone left in atari makes the captured point the ko point — the opponent may
//     not retake there on the next move.  summarize(out, true) marks it in the stored
//     liberty plane as KO_MARK at that EMPTY point (the plane is 0 at every empty point
//     otherwise, so 9-plane files keep their shape and a reader that gates the liberty
//     planes on a stone — every expander here does — sees the reference's 37 planes).
//   * liberties_after / kills (count_kills_and_liberties :304-327)
//   * group liberties (all_ladder_moves_and_liberties :441-479)
//   * ladders (ladder_moves :393-439, recursive) — group size written for the attacker,
//     later groups in row-major scan order overwrite earlier ones
//   * age (update_board :329-354): +1 on every point with 0 < age < 255, then 1 on the
//     played point and every cleared point.
// The board is a flat array indexed x*19 + y (x = first SGF coordinate, 0-based), i.e.
// the reference's hash(x, y) (:188-196).  Flood fills use a stamp-marked visited array
// instead of Lua hash tables.
#pragma once
#include <array>
#include <cstdint>
#include <stdexcept>
#include <vector>

namespace dg {

constexpr int N = 19;
constexpr int NN = N * N;

struct Move {
  int player;  // 1 black, 2 white
  int x, y;    // 0-based
};

// Stored planes of one position, layout [plane][x][y] (dataloader.lua:20-27).
enum Plane : int {
  P_STONES = 0, P_LIBS = 1, P_LIBS_AFTER_B = 2, P_LIBS_AFTER_W = 3, P_KILLS_B = 4,
  P_KILLS_W = 5, P_AGE = 6, P_LADDER_B = 7, P_LADDER_W = 8, NUM_STORED = 9
};

// liberty-plane value at the simple-ko point (summarize(out, mark_ko=true))
constexpr uint8_t KO_MARK = 255;

class IllegalMove : public std::runtime_error {
 public:
  using std::runtime_error::runtime_error;
};

class Board {
 public:
  Board();
  void clear();
  uint8_t at(int idx) const { return s_[idx]; }
  const std::array<uint8_t, NN>& stones() const { return s_; }
  const std::array<uint8_t, NN>& ages() const { return age_; }
  void set_stones(const uint8_t* stones);  // 361 values in {0,1,2}; ages untouched, no ko
  // simple-ko point left by the last play() (-1: none)
  int ko() const { return ko_; }

  // Real move with captures and ageing (update_board).  Throws IllegalMove on an
  // occupied point.
  void play(const Move& m);

  // Liberty count of the group at idx (0 for an empty point) and optionally the group
  // members / liberty points.
  int liberties(int idx, std::vector<int>* group = nullptr, std::vector<int>* libs = nullptr);

  // Trial play of `player` at empty idx: returns (kills, liberties of the played stone's
  // group afterwards), board restored on return.
  void kills_and_liberties(int idx, int player, int* kills, int* libs_after);

  // Compute the 9 stored planes for the current position into out[9*361]
  // (age plane = current ages; mark_ko: KO_MARK in the liberty plane at the ko point).
  void summarize(uint8_t* out, bool mark_ko = false);

  // Trial play of `player` at empty idx as kills_and_liberties, returning also the XOR of the
  // Zobrist keys (position_key) of the position after the play and the position now.
  uint64_t trial_key_delta(int idx, int player, int* kills, int* libs_after);

  // A move that places no stone (Game::pass_): ages advance as for a move, no ko point.
  void pass();
  // Put back a position recorded from stones() / ages() / ko() (Game::undo).
  void restore(const std::array<uint8_t, NN>& stones, const std::array<uint8_t, NN>& ages,
               int ko);

  // Number of ladder-search nodes visited by the last summarize() (diagnostics).
  long long ladder_nodes() const { return ladder_nodes_; }

 private:
  struct Undo {
    int idx;
    uint8_t prev;
  };
  void put(int idx, uint8_t v, std::vector<Undo>* log);
  // play_with_f: place + resolve captures; `removed_opp` counts cleared opponent stones.
  void place_and_resolve(int idx, int player, std::vector<Undo>* log, int* removed_opp,
                         std::vector<int>* cleared);
  void unwind(std::vector<Undo>& log, size_t to);
  bool ladder_moves(int gx, const int libs2[2], std::vector<int>* result, int depth);

  std::array<uint8_t, NN> s_{};
  std::array<uint8_t, NN> age_{};
  // flood-fill scratch
  std::array<uint32_t, NN> mark_{};
  std::array<uint32_t, NN> lmark_{};
  uint32_t stamp_ = 0;
  std::vector<int> stack_;
  long long ladder_nodes_ = 0;
  int ko_ = -1;
};

// Plays a whole game: optional handicap stones, then the moves; for each move emits the
// stored planes of the position BEFORE it (all_boards, makedata.lua:156-186).
// out: [num_moves][9][361]; returns number of positions written.  Throws IllegalMove.
// mark_ko: each position's simple-ko point marked (Board::summarize).
int game_positions(const std::vector<Move>& handicap, const std::vector<Move>& moves,
                   uint8_t* out, bool mark_ko = false);

// Zobrist key of a stone of `colour` (1, 2) at idx: a fixed table filled at start-up by
// splitmix64 from a fixed seed, so keys are the same in every process.  position_key: the XOR
// over all stones (0 for the empty board); the side to move is not part of it.
uint64_t zobrist(int colour, int idx);
uint64_t position_key(const std::array<uint8_t, NN>& stones);

// A live game: a Board, the side to move and the history of everything a move changes, so
// undo() is exact.  Board's rules are unchanged (suicide is playable and ko is not enforced by
// play()); what a player may do is legal_mask()'s business.
class Game {
 public:
  Game();
  void clear();
  // A stone of `player` at (x, y), 0-based; throws IllegalMove on an occupied point or off the
  // board.  The other colour is then to move.
  void play(int player, int x, int y);
  // `player` passes: the ko point is cleared and ages advance as for a move.
  void pass_(int player);
  // Take back the last play() / pass_(): stones, ages, ko, side to move and history bit for
  // bit.  False (and no change) at the start of the game.
  bool undo();

  int to_move() const { return to_move_; }
  int ply() const { return (int)hist_.size(); }
  bool last_was_pass() const { return !hist_.empty() && hist_.back().was_pass; }
  const Board& board() const { return b_; }
  int ko() const { return b_.ko(); }
  uint64_t key() const { return keys_.back(); }

  // Board::summarize of the current position into out[9*361].
  void planes(uint8_t* out, bool mark_ko = false) { b_.summarize(out, mark_ko); }

  // out[361], nonzero = `player` may not play there.  Always: occupied points and the
  // simple-ko point.  !suicide: points whose trial play kills nothing and leaves the played
  // group without a liberty.  superko: points whose resulting position repeats an earlier
  // position of this game, the current one included (positional superko, by Zobrist key).
  // !eye_fill: the player's own simple eyes (simple_eye).
  void legal_mask(int player, bool suicide, bool superko, bool eye_fill, uint8_t* out);

  // An empty point whose on-board orthogonal neighbours are all `player`'s stones and of whose
  // on-board diagonal neighbours at most one is not `player`'s stone (none on the edge or in a
  // corner).
  bool simple_eye(int idx, int player) const;

  // Tromp-Taylor area: stones plus the empty regions that reach only that colour.
  void score(int* black, int* white) const;

 private:
  struct Entry {   // the state before the move
    std::array<uint8_t, NN> stones, ages;
    int ko, to_move;
    bool was_pass;
  };
  Board b_;
  int to_move_ = 1;
  std::vector<Entry> hist_;
  std::vector<uint64_t> keys_;   // of the start position and of the position after every move
};

// Neighbour table in the reference's order: (-1,0), (1,0), (0,-1), (0,1).
extern int g_nbr[NN][4];
extern int g_nnbr[NN];

}  // namespace dg
