// The slab feed of the CTC lattice drivers (engine.h: CtcAligner, CtcGraphAligner, CtcScorer, CtcFinder), host code only.
// The kernels see the log-probs one slab of rows [r0, r0 + nrows) at a time.  Every sequence owns an increasing list of rows (its
// frames; the rows between two chunks' valid frames are padding and belong to nobody), and a slab advances the sequence over the
// frames [f0, f1) whose rows it holds.  Seq is any descriptor with frame_off, T, f0, f1 (VitSeq, GraphSeq, FindSeq); h_rows holds the
// row lists back to back, a sequence's at its frame_off.  A driver adds its own checks, its buffers and the kernel launch.
#pragma once
#include <algorithm>
#include <limits>
#include <string>
#include <utility>
#include <vector>

#include "common.h"

namespace rvb {

// plan(): a sequence's frame count against the cap.  at: the caller's "who: sequence i: "; unit: what the cap is counted per
inline int slab_frame_cap(const std::string& at, int64_t T, int64_t cap, const char* unit) {
  if (T <= cap) return OK;
  set_error(at + std::to_string(T) + " frames exceed the cap of " + std::to_string(cap) + " frames per " + unit);
  return E_UNSUPPORTED;
}

// plan(): a sequence's rows, which must increase, go to the end of h_rows and count into frame_off (what: all that the caller
// holds against the same bound)
inline int slab_take_rows(const std::string& who, const std::string& at, const std::vector<int32_t>& rows, std::vector<int32_t>* h_rows,
                          int64_t* frame_off, const char* what = "frames") {
  for (size_t f = 1; f < rows.size(); ++f)
    if (rows[f] <= rows[f - 1]) { set_error(at + "frame rows must increase"); return E_ARG; }
  h_rows->insert(h_rows->end(), rows.begin(), rows.end());
  *frame_off += (int64_t)rows.size();
  if (*frame_off > std::numeric_limits<int32_t>::max() / 2) { set_error(who + ": too many " + what + " in one call"); return E_UNSUPPORTED; }
  return OK;
}

// the frames {f0, f1} of q whose rows lie in [r0, r0 + nrows); f0 == f1 when the slab holds none
template <typename Seq> std::pair<int, int> slab_frames(const Seq& q, const std::vector<int32_t>& h_rows, int r0, int nrows) {
  const int32_t* rw = h_rows.data() + q.frame_off;
  return {(int)(std::lower_bound(rw, rw + q.T, r0) - rw), (int)(std::lower_bound(rw, rw + q.T, r0 + nrows) - rw)};
}

// does the slab hold a frame of any sequence?  (a slab of padding rows only is not even computed)
template <typename Seq> bool slab_touches(const std::vector<Seq>& seq, const std::vector<int32_t>& h_rows, int r0, int nrows) {
  for (const Seq& q : seq) {
    const auto [f0, f1] = slab_frames(q, h_rows, r0, nrows);
    if (f0 < f1) return true;
  }
  return false;
}

// One step of a sweep: every sequence's window [f0, f1) of this slab.  Ascending (a sweep from f0 = f1 = 0): a sequence the slab does
// not touch gets the empty window [f1, f1) where it stands, and one it touches must continue there, else the slab came twice or out
// of order.  Descending (from f0 = f1 = T): the mirror image, [f0, f0) and a window that ends where the sequence stands.
// *any: there is a frame to advance over, i.e. something to launch.
template <typename Seq>
int slab_window(const char* who, bool descending, std::vector<Seq>& seq, const std::vector<int32_t>& h_rows, int r0, int nrows, bool* any) {
  *any = false;
  for (Seq& q : seq) {
    const auto [f0, f1] = slab_frames(q, h_rows, r0, nrows);
    const int at = descending ? q.f0 : q.f1;
    if (f0 == f1) { q.f0 = q.f1 = at; continue; }
    if ((descending ? f1 : f0) != at) {
      set_error(std::string(who) + (descending ? ": the backward sweep takes the slabs in descending row order" : ": slabs must arrive in row order"));
      return E_STATE;
    }
    q.f0 = f0; q.f1 = f1;
    *any = true;
  }
  return OK;
}

// finish(): has the ascending sweep reached the last frame of every sequence, the descending one the first?
template <typename Seq> int slab_covered(const char* who, bool descending, const std::vector<Seq>& seq) {
  for (const Seq& q : seq)
    if (descending ? q.f0 != 0 : q.f1 != q.T) {
      set_error(std::string(who) + (descending ? ": the backward sweep did not reach the first frame of a sequence"
                                               : ": the slabs did not cover every frame of a sequence"));
      return E_STATE;
    }
  return OK;
}

// finish(): a lattice whose score is -inf has no path that `does` ("emits the transcript", ...)
template <typename Seq, typename F> int slab_feasible(const char* who, const std::vector<Seq>& seq, const F* score, const char* does) {
  for (size_t i = 0; i < seq.size(); ++i)
    if (!(score[i] > -INFINITY)) {
      set_error(std::string(who) + ": sequence " + std::to_string(i) + ": infeasible: no path of " + std::to_string(seq[i].T) + " frames " +
                does + " with a finite score");
      return E_ARG;
    }
  return OK;
}

// the descriptors of one launch: a synchronous copy, so the host vector may change for the next slab
template <typename Seq> int slab_upload(hipStream_t s, void* d_seqs, const std::vector<Seq>& seq) {
  RVB_HIP_CHECK(hipStreamSynchronize(s));
  RVB_HIP_CHECK(hipMemcpy(d_seqs, seq.data(), seq.size() * sizeof(Seq), hipMemcpyHostToDevice));
  return OK;
}

}  // namespace rvb
