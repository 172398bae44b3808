// pause_chunks.hip: cut transcription chunks at pauses (rvb_pause_chunks; the definition is in include/rvb.h).
#pragma once
#include <cstdint>

#include <hip/hip_runtime.h>

namespace rvb {

constexpr int PAUSE_MAX_SMOOTH = 64;      // largest smoothing half-width h

// One recording of a pause search: its frame j is row row0 + j of the features; its piece starts go to table[tab0 ..) (tab_cap
// entries: pause_max_pieces).
struct PauseRec {
  int64_t row0;
  int64_t tab0;
  int32_t n_frames;
  int32_t tab_cap;
};
// One piece of the gather: `len` rows from row `src` on.
struct PausePiece {
  int64_t src;
  int32_t len;
  int32_t reserved;
};

// The most pieces the definition can cut n frames into: every piece but the last has at least chunk_size - search frames.
inline int64_t pause_max_pieces(int64_t n, int chunk_size, int search) {
  return n <= 0 ? 0 : n <= chunk_size ? 1 : (n + (chunk_size - search) - 1) / (chunk_size - search);
}

// RVB_E_ARG, in `who`'s name, unless 1 <= h <= PAUSE_MAX_SMOOTH, chunk_size >= 7 and 7 <= search <= chunk_size - 7
int pause_check_args(const char* who, int chunk_size, int search, int h);

// e[row] = fp32 sum of the 80 log-mel values of every live frame (recording r owns the launch's frames [frame0[r], frame0[r + 1])).
// frame0 [n_rec + 1] and rec [n_rec] are device arrays; rows of `loud` that hold no live frame are not written.
int pause_loudness(hipStream_t s, const float* feats, const int64_t* frame0, const PauseRec* rec, int n_rec, int64_t total_frames,
                   float* loud);
// One workgroup per recording walks it serially: table[rec[r].tab0 + k] = start of piece k, count[r] = its pieces.
int pause_cuts(hipStream_t s, const float* loud, const PauseRec* rec, int n_rec, int chunk_size, int search, int h, int32_t* table,
               int32_t* count);
// Piece k's rows -> rows [k * chunk_size, k * chunk_size + len) of out, the rest of the slot zero.  pieces [n_pieces] on the device.
int pause_gather(hipStream_t s, const float* feats, const PausePiece* pieces, int64_t n_pieces, int chunk_size, float* out);

}  // namespace rvb
