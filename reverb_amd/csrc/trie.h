// The rescoring trie: its builder and the stitching of per-chunk tries (engine_decode.hip; test_api.hip checks one against the other).
#pragma once
#include <algorithm>
#include <utility>
#include <vector>

#include "engine.h"

namespace rvb {

// The n-best hypotheses of a chunk share long prefixes (they come out of one prefix beam), and the decoder is causal:
// decoder row j of a hypothesis depends only on its tokens 0..j-1 and on the chunk's memory.  The reference runs the
// decoder on the padded [N, L] batch (search.py:391-412, asr_model.py:868-978), i.e. it recomputes a shared prefix N
// times; here every DISTINCT prefix of a chunk is one decoder row (a trie, built per decoder direction: the
// right-to-left decoder sees the reversed hypotheses, search.py:427-433).  Row results do not depend on the batch they
// are computed in (GEMM rows are independent, an attention row walks its own keys in order), so every hypothesis
// reads exactly the log-probs the padded batch would give it.  On the bench workload 13-35 % of the rows remain.
// seq(h, j) = j-th decoder input token AFTER <sos> of hypothesis h; target of pair (h, j) = seq(h, j) for j < len, else eos
template <typename SeqFn>
void build_trie_range(const HypRef* hb, const HypRef* he, int chunk0, int B, int sos, int eos, SeqFn seq, TrieBatch* t) {
  *t = TrieBatch();
  std::vector<std::pair<int32_t, int32_t>> asks;   // (row, target) in pair order
  std::vector<std::vector<std::pair<int32_t, int32_t>>> kids;   // per row: (token, child row) -- fan-out is tiny
  t->crow_start.assign(B, 0); t->crow_len.assign(B, 0);
  int cur_chunk = -1, root = -1;
  for (const HypRef* hp = hb; hp != he; ++hp) {
    const HypRef& h = *hp;
    if (h.chunk - chunk0 != cur_chunk) {
      if (cur_chunk >= 0) t->crow_len[cur_chunk] = t->R - t->crow_start[cur_chunk];
      cur_chunk = h.chunk - chunk0;
      t->crow_start[cur_chunk] = t->R;
      root = -1;
    }
    const int first_new = t->R;
    int own_pos0 = -1;
    t->hkv_start.push_back((int32_t)t->path.size());
    int node = root;
    for (int j = 0; j <= h.len; ++j) {
      int next = -1;
      if (j == 0) {
        next = root;
      } else {
        const int tk = seq(h, j - 1);
        for (auto& kv : kids[node]) if (kv.first == tk) { next = kv.second; break; }
      }
      if (next < 0) {
        next = t->R++;
        t->tok.push_back(j == 0 ? sos : seq(h, j - 1));
        t->pos.push_back(j);
        kids.emplace_back();
        if (j == 0) root = next; else kids[node].push_back({seq(h, j - 1), next});
        if (own_pos0 < 0) own_pos0 = j;
      }
      node = next;
      t->path.push_back(node);
      asks.push_back({node, j < h.len ? seq(h, j) : eos});
    }
    const int n_own = t->R - first_new;             // new rows are a suffix of the path and contiguous
    t->hq_start.push_back(first_new); t->hq_len.push_back(n_own); t->hq_pos0.push_back(n_own ? own_pos0 : 0);
    t->hkv_len.push_back(h.len + 1);
    for (int q0 = 0; q0 < n_own; q0 += 16) { t->work.push_back((int32_t)t->hq_start.size() - 1); t->work.push_back(q0); }
  }
  if (cur_chunk >= 0) t->crow_len[cur_chunk] = t->R - t->crow_start[cur_chunk];
  for (int b = 0; b < B; ++b) t->max_chunk_rows = std::max(t->max_chunk_rows, t->crow_len[b]);
  // CSR of the asks by row (counting sort keeps pair order inside a row)
  t->P = (int)asks.size();
  t->tgt_ptr.assign(t->R + 1, 0);
  for (auto& a : asks) t->tgt_ptr[a.first + 1]++;
  for (int r = 0; r < t->R; ++r) t->tgt_ptr[r + 1] += t->tgt_ptr[r];
  std::vector<int32_t> fill(t->tgt_ptr.begin(), t->tgt_ptr.end() - 1);
  t->tgt.assign(t->P, 0); t->pair_slot.assign(t->P, 0);
  for (int p = 0; p < t->P; ++p) { const int slot = fill[asks[p].first]++; t->tgt[slot] = asks[p].second; t->pair_slot[p] = slot; }
}

// The batch trie from the chunks' tries: the rows of a chunk are contiguous and only that chunk's hypotheses refer to them, so
// a chunk's local numbering differs from the global one by the running totals of the chunks before it -- rows, hypotheses,
// path entries, (hypothesis, position) pairs.  Bit-identical to build_trie_range over all hypotheses at once (which took
// 1.6 ms on one thread for the 176-chunk bench batch, with the device idle).
inline void merge_tries(const std::vector<TrieBatch>& part, TrieBatch* t) {
  const int B = (int)part.size();
  *t = TrieBatch();
  size_t nR = 0, nH = 0, nPath = 0, nP = 0, nW = 0;
  for (const TrieBatch& c : part) { nR += c.R; nH += c.hq_start.size(); nPath += c.path.size(); nP += c.P; nW += c.work.size(); }
  t->tok.reserve(nR); t->pos.reserve(nR); t->path.reserve(nPath); t->work.reserve(nW);
  t->hq_start.reserve(nH); t->hq_len.reserve(nH); t->hq_pos0.reserve(nH); t->hkv_start.reserve(nH); t->hkv_len.reserve(nH);
  t->tgt.reserve(nP); t->pair_slot.reserve(nP); t->tgt_ptr.reserve(nR + 1);
  t->crow_start.assign(B, 0); t->crow_len.assign(B, 0);
  for (int b = 0; b < B; ++b) {
    const TrieBatch& c = part[b];
    const int32_t R0 = t->R, H0 = (int32_t)t->hq_start.size(), PATH0 = (int32_t)t->path.size(), P0 = t->P;
    t->crow_start[b] = c.R ? R0 : 0; t->crow_len[b] = c.R;      // a chunk without hypotheses keeps the zeros of the batch form
    t->max_chunk_rows = std::max(t->max_chunk_rows, c.R);
    t->tok.insert(t->tok.end(), c.tok.begin(), c.tok.end());
    t->pos.insert(t->pos.end(), c.pos.begin(), c.pos.end());
    for (int32_t v : c.path) t->path.push_back(v + R0);
    for (int32_t v : c.hq_start) t->hq_start.push_back(v + R0);
    t->hq_len.insert(t->hq_len.end(), c.hq_len.begin(), c.hq_len.end());
    t->hq_pos0.insert(t->hq_pos0.end(), c.hq_pos0.begin(), c.hq_pos0.end());
    for (int32_t v : c.hkv_start) t->hkv_start.push_back(v + PATH0);
    t->hkv_len.insert(t->hkv_len.end(), c.hkv_len.begin(), c.hkv_len.end());
    for (size_t k = 0; k + 1 < c.work.size(); k += 2) { t->work.push_back(c.work[k] + H0); t->work.push_back(c.work[k + 1]); }
    for (int r = 0; r < c.R; ++r) t->tgt_ptr.push_back(c.tgt_ptr[r] + P0);
    t->tgt.insert(t->tgt.end(), c.tgt.begin(), c.tgt.end());
    for (int32_t v : c.pair_slot) t->pair_slot.push_back(v + P0);
    t->R += c.R; t->P += c.P;
  }
  t->tgt_ptr.push_back(t->P);
}

}  // namespace rvb
