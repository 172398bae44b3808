/* test_api.h -- entry points of librvb_test.so: raw kernel / host-search hooks for the unit tests and the tuning scripts
 * (host buffers in, host buffers out).  NOT part of the product: librvb.so exports include/rvb.h and include/rvd.h only;
 * reverb_amd/build.py links the same objects plus csrc/test_api.hip (in place of the product's csrc/lab_env_off.cpp) into
 * reverb_amd/librvb_test.so, which tests/ and scripts/ load through reverb_amd._lib.load_test(). */
#ifndef RVB_TEST_API_H_
#define RVB_TEST_API_H_
#include "../../include/rvb.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- raw kernel entry points for unit tests (host buffers in, host buffers out) ---- */
int rvb_test_gemm(int dtype, const float* A, const float* W, const float* bias, const float* res, float* C,
                  int M, int N, int K, float alpha, int act, int out_f32,
                  int conv, int cT1, int cF1, int cC, int cB);
int rvb_test_rownorm(int dtype, const float* x, const float* gamma, const float* beta, float eps, int mode,
                     int silu, const float* add, float* out, int out_f32, int M, int d);
/* conv_block.hip (a whole 32-channel BasicBlock per launch) on host floats, unbordered NHWC in / out, torch weight layout */
int rvb_test_conv_block32(const float* x, const float* wa, const float* ba, const float* wb, const float* bb, float* out, int B, int F, int T);
// conv_s2.hip on a plane of its own: x [B][Fi][Ti][32], w [64][32][3][3], wsc [64][32] -> out = relu(conv3x3 stride 2) and sc = conv1x1 stride 2, [B][Fo][To][64]
int rvb_test_conv_s2sc(const float* x, const float* w, const float* b, const float* wsc, const float* bsc, float* out, float* sc, int B, int Fi, int Ti);
int rvb_test_conv1(int dtype, const float* feats, const float* mean, const float* istd, const float* w,
                   const float* b, float* out, int B, int T0, int F0, int d);
/* round-4 candidate: the fp8 implicit-GEMM convolution (csrc/conv_gemm.hip conv_igemm8_kernel) on host floats, see test_api.hip */
int rvb_test_conv_igemm_fp8(const float* x, const float* w, const float* bias, const float* res, float* out, float* out8, int B,
                            int Fi, int Ti, int Cin, int Cout, int stride, int relu, float a_scale, float out8_scale, float* x_deq,
                            float* w_deq, float* amax);
/* host only: the `joint_decoding` state machine of one chunk (csrc/search.cpp JointSearch: transformer/search.py:450-496,
 * espnet/beam_search_timesync.py), driven frame by frame; the caller supplies the attention log-probs it asks for */
void* rvb_test_joint_new(int beam, int pre_beam, int blank, int sos, double w_ctc, double w_dec, double bonus);
void rvb_test_joint_free(void* h);
int rvb_test_joint_begin(void* h, int t, const float* tv, const int32_t* ti, int K, float p_tok0, float p_blank, int32_t* decode,
                         int32_t* n_decode, int32_t* pair_node, int32_t* pair_tok, int32_t* n_pairs, int cap);
int rvb_test_joint_finish(void* h, const float* vals);
int rvb_test_joint_prefix(void* h, int node, int32_t* toks, int32_t* n);
int rvb_test_joint_result(void* h, int32_t* tokens, int32_t* times, int32_t* end_times, double* conf, int32_t* n, double* score);
/* `causal`: bit 0 causal, bit 1 bf16 output (bf16 engine), bit 2 the gated form: G is [B][T][d], already a * sigmoid(b) (what the
 * pointwise GEMM's ACT_GLU epilogue stores) */
int rvb_test_glu_dwconv(int dtype, const float* G, const float* pw1_bias, const float* dw_w, const float* dw_b,
                        const int32_t* lens, float* out, int B, int T, int d, int K, int causal,
                        const float* hist /* nullable [K-1][2d] */, int hist_rows);
/* dwconv_ln() of the bf16 engine on host floats: G [B][T][d] gated, dw_w [d][K] as the reference stores it, xn [B][T][d] = SiLU(LayerNorm(
 * depthwise conv)).  grid > 0 launches that many workgroups (short row ranges that begin and end anywhere), 0 the launcher's own
 * choice.  xn_two / dconv_two (nullable): the same inputs through glu_dwconv (gated, bf16 output) and rownorm (LayerNorm + SiLU on
 * the bf16 input), and the tensor between the two.  Every device output starts as all-ones bytes (NaN). */
int rvb_test_dwconv_ln(const float* G, const float* pw1_bias, const float* dw_w, const float* dw_b, const int32_t* lens,
                       const float* gamma, const float* beta, float eps, float* xn, float* xn_two, float* dconv_two, int B, int T,
                       int d, int K, int grid);
int rvb_test_attention(int dtype, const float* q, const float* k, const float* v, const float* p,
                       const float* bias_u, const float* bias_v, float* out, int q_rows, int kv_rows, int p_rows,
                       int heads, int dk, const int32_t* q_start, const int32_t* q_len, const int32_t* kv_start,
                       const int32_t* kv_len, int nseq, int causal);
/* decoder self attention over shared prefixes: sequence s has kv_len[s] keys in rows kv_index[kv_start[s] ..] and
 * q_len[s] queries in rows q_start[s] .. at key positions q_pos0[s] .. (causal); q_block 16 = one-wave blocks + work list */
int rvb_test_attention_trie(int dtype, const float* q, const float* k, const float* v, float* out, int rows, int heads, int dk,
                            const int32_t* q_start, const int32_t* q_len, const int32_t* q_pos0, const int32_t* kv_start,
                            const int32_t* kv_len, const int32_t* kv_index, int n_index, int nseq, int q_block);
/* attention() with everything AttnArgs carries, on host floats, so that a test can build any call the engine builds.
 * q / k / v / out are (buffer [rows][stride], column offset of head 0): buffers given by the same host pointer are uploaded once, so
 * q, k, v may share the fused qkv buffer (stride 3d, columns 0 / d / 2d) or k, v one of stride 2d.  `out` goes up as the caller filled
 * it and comes back whole: columns the kernel does not own keep their sentinel.  The kernel reads positional row p_off + j for key j;
 * fold = 1 builds the per-key table with attention_pos_bias from row p_off on (p_rows - p_off entries per head) and passes
 * fold_kv_cap / k_prefolded as given (prefolded: `k` holds k + p already).  max_q 0 = the longest q_len.  lab = ATTN_LAB_* bits
 * (1 = three workgroups per CU, 2 = one fragment per wave, 4 = 16-byte K row pad).  ran[8] = the instantiation that was chosen:
 * {element size, DKP, HAS_POS, NW, FOLD, PADK, OCC, MF}, zeros when none was launched.  Every index, stride and kv_index entry is
 * checked against the buffer sizes before any device work (E_ARG). */
typedef struct rvb_test_attn_args {
  int32_t dtype, heads, dk, nseq;
  const float* q; int32_t q_rows, q_stride, q_col, pad0;
  const float* k; int32_t k_rows, k_stride, k_col, pad1;
  const float* v; int32_t v_rows, v_stride, v_col, pad2;
  float* out; int32_t o_rows, o_stride, o_col, pad3;
  const float* p; int32_t p_rows, p_stride, p_col, p_off;
  const float* bias_u; const float* bias_v;
  const int32_t* q_start; const int32_t* q_len; const int32_t* kv_start; const int32_t* kv_len;
  const int32_t* q_pos0; const int32_t* kv_index; const int32_t* work;
  int32_t n_index, n_work, max_q, q_block, causal, chunk, left, plain_order, fold, k_prefolded, fold_kv_cap, lab;
  int32_t ran[8];
} rvb_test_attn_args;
int rvb_test_attention_ex(rvb_test_attn_args* a);
/* attention_pos_bias on its own: the fp32 table out[heads][p_rows - p_off] of positional rows p_off.. of p [p_rows][p_stride] */
int rvb_test_attention_pos_bias(const float* p, int p_rows, int p_stride, int p_col, int p_off, const float* bias_u, const float* bias_v,
                                int heads, int dk, float scale, float* out);
int rvb_test_logsoftmax_topk(const float* logits, int M, int V, int k, float blank_penalty, int blank_id,
                             float* topk_val, int32_t* topk_idx, float* logp);
int rvb_test_lse_gather(const float* logits, int R, int V, const int32_t* target, float* out);
/* the three entry points of softmax_topk.hip's row_lse_kernel as the engine calls them: host logits [M][ld] with the pad columns
 * V .. ld - 1 as the caller filled them (the kernel must not read them), the blank penalty and blank id of kernels.h (lse_gather_multi
 * has none).  logp [M][V] stays nullable.  The device outputs start as all-ones bytes (NaN / -1), so an element the kernel did not
 * write comes back as that.  Refused by name before any device work: V < 1, ld < V, a target outside [0, V), a ptr that does not
 * ascend from 0; what the launcher refuses (k outside [1, 64], k > V) leaves the outputs as the caller filled them.  The three hooks
 * without a stride are the ld = V, no-penalty calls of these. */
int rvb_test_logsoftmax_topk_ex(const float* logits, int M, int V, int ld, int k, float blank_penalty, int blank_id,
                                float* topk_val /* [M][k] */, int32_t* topk_idx /* [M][k] */, float* logp);
int rvb_test_lse_gather_ex(const float* logits, int R, int V, int ld, const int32_t* target /* [R] */, float blank_penalty, int blank_id,
                           float* out /* [R] */);
int rvb_test_lse_gather_multi_ex(const float* logits, int R, int V, int ld, const int32_t* ptr /* [R+1] */, const int32_t* target,
                                 float* out /* [ptr[R]] */);
/* fp8 (e4m3) GEMM / LayerNorm-to-fp8 of the RVB_FP8 mode on host floats (operands quantised as the engine does) */
/* bf16 GEMM with bf16 output and the row-periodic addend of GemmArgs::rowadd (round 6): C[m][n] = A.W^T + bias (+ add[m % add_rows][n - add_col0]
 * for add_col0 <= n < add_col0 + add_cols); add is fp32 on the host, rounded to bf16 on the way up (what the engine's positional keys are) */
int rvb_test_gemm_glu(const float* A, const float* W, const float* bias, float* C, int M, int N, int K);
int rvb_test_gemm_rowadd(const float* A, const float* W, const float* bias, const float* add, float* C, int M, int N, int K,
                         int add_rows, int add_col0, int add_cols);
/* csrc/mp3.cpp (round 6).  decode: as rvb_audio_decode_f32 + the stream facts (info9: version, channels, rate, audio frames, samples per
 * frame, info frame, start skip, samples, kbit/s) and what the pass saw (stats12: granule-channels, Huffman data ending exactly on /
 * before / past part2_3_length, CRCs checked / failed, frames without their reservoir bytes, short / mixed / M-S / intensity granules,
 * largest main_data_begin).  hybrid / polyphase: one granule of the two synthesis stages on caller state.  window: D[512].
 * huffman: table t of the standard (32 / 33 = count1 A / B) -> number of entries, (code, length) per symbol, linbits per table_select. */
int64_t rvb_test_mp3_decode(const void* data, int64_t nbytes, int channel, float* out, int64_t capacity, int64_t* info9, int64_t* stats12, int threads);
int rvb_test_mp3_hybrid(float* xr576, float* overlap576, int block_type, int mixed, float* out576);
int rvb_test_mp3_polyphase(const float* sb576, float* vbuf1024, int* voff, float* pcm576);
int rvb_test_mp3_window(float* out512);
int rvb_test_mp3_huffman(int t, uint16_t* codes, uint8_t* lens, int32_t* linbits32);
int rvb_test_gemm_fp8(const float* A, const float* W, const float* bias, const float* res, float* C, int M, int N, int K,
                      float a_scale, float alpha, int act, int out_kind, float out_scale, float* a_deq, float* w_deq);
/* gemm() with everything GemmArgs carries but the row-periodic addend, on host floats, so that a test can build any call the engines
 * build (run_gemm: strides, a null bias, the residual in the output buffer, A offset into its allocation, overlapping rows).
 * A: a_elems values, rounded to the compute dtype (or quantised to e4m3 at a_scale when in_fp8); the kernel's A starts a_row0 * lda
 * elements in, so a_elems >= (a_row0 + M - 1) * lda + K (lda < K: overlapping rows); conv != 0: the NHWC activation of rvb_test_gemm
 * (lda = cC, a_row0 = 0, a_elems ignored).  W [N][ldw] (in_fp8: one scale per row, as rvb_test_gemm_fp8 quantises).  bias [N] and
 * res [M][ldres] are nullable.  C [c_rows][ldc] (c_rows 0 = M, else >= M) goes up as the caller filled it and comes back whole:
 * pad columns and rows past M keep their canaries.  The output is fp32 (f32 engine, out_f32), e4m3 of value / out_scale (out_fp8;
 * a NaN of the caller's goes up as the NaN code and comes back NaN) or bf16.  inplace: the fp32 output buffer IS the residual (res
 * null, ldres ignored in favour of ldc).  a_deq [a_elems] / w_deq [N][ldw] (nullable, in_fp8 only): the values the quantised operands
 * stand for.  path (out): 2 when gemm() hands this problem to gemm2.hip (gemm2_applicable and the variant switch), else 1.
 * Refused by name before any device work (E_ARG): a buffer smaller than the strides need, inplace without an fp32 output.  What gemm()
 * itself refuses comes back with its code and its words, C as the caller filled it. */
typedef struct rvb_test_gemm_args {
  int32_t dtype, M, N, K, lda, ldw, ldc, ldres;
  int32_t act, out_f32, out_fp8, in_fp8, inplace, a_row0, c_rows, conv;
  int32_t cT1, cF1, cC, cB;
  float alpha, a_scale, out_scale;
  int32_t path;
  int64_t a_elems;
  const float* A; const float* W; const float* bias; const float* res;
  float* C; float* a_deq; float* w_deq;
} rvb_test_gemm_args;
int rvb_test_gemm_ex(rvb_test_gemm_args* a);
int rvb_test_rownorm_fp8(const float* x, const float* gamma, const float* beta, float eps, int silu, int M, int d, float scale,
                         float* out, const float* gamma2, const float* beta2, float eps2, float scale2, float* out1_f32, float* out2);
/* rownorm() with everything NormArgs carries, on host floats.  x goes up as fp32, or as bf16 when x_bf16; add in the compute dtype.
 * out: bf16 (bf16 engine), fp32 (f32 engine or out_f32) or e4m3 of value / out_scale (out_fp8).  gamma2 non-null adds the fused second
 * LayerNorm: out2 in the compute dtype, or e4m3 of value / out2_scale (out2_fp8).  fp8 outputs come back de-quantised as
 * rvb_test_rownorm_fp8 returns them.  The device outputs start as all-ones bytes (a NaN in every output format), so an element the
 * kernel did not write comes back NaN; when the launcher refuses the call, out / out2 are left as the caller filled them.
 * sat / sat2 = the two saturation counters after the call. */
typedef struct rvb_test_norm_args {
  int32_t dtype, x_bf16, mode, silu, out_f32, out_fp8, out2_fp8, M, d, pad0;
  float eps, eps2, out_scale, out2_scale;
  const float* x; const float* gamma; const float* beta; const float* add; const float* gamma2; const float* beta2;
  float* out; float* out2;
  uint32_t sat, sat2;
} rvb_test_norm_args;
int rvb_test_rownorm_ex(rvb_test_norm_args* a);
/* subsample_conv1 with its fp8 output (out_fp8_scale > 0: out comes back de-quantised), the running maximum (amax nullable: in = the
 * slot's initial value, out = the slot after the call) and the saturation counter (sat nullable).  w as rvb_test_conv1 takes it. */
int rvb_test_conv1_ex(int dtype, const float* feats, const float* mean, const float* istd, const float* w, const float* b, float* out,
                      int B, int T0, int F0, int d, float out_fp8_scale, float* amax, uint32_t* sat);
/* embed_tokens: out[r] = E[tok[r]] * scale + pe[pos[r]]; E [vocab][d], pe [n_pos][d]; indices outside the tables are refused */
int rvb_test_embed(const float* E, int vocab, const float* pe, int n_pos, const int32_t* tok, const int32_t* pos, float* out, int rows,
                   int d, float scale);
/* amax_abs over n values (rounded to bf16 on the way up in the bf16 engine); *slot in = the slot's initial value, out = the slot */
int rvb_test_amax_abs(int dtype, const float* x, int64_t n, float* slot);
/* convert_f32: dst = the n values as the compute dtype holds them (bf16 widened back to fp32, bit for bit) */
int rvb_test_convert_f32(int dtype, const float* src, float* dst, int64_t n);
/* gather_cache on caches [R][L][row_bytes]: dst goes up as the caller filled it and comes back whole */
int rvb_test_gather_cache(const void* src, void* dst, const int32_t* parent, int R, int L, int rows, int row_bytes);
/* softmax_topk.hip gather_pairs: out[i] = table[row[i]][col[i]], table fp32 [rows][ld]; pairs outside the table are refused; out goes up
 * as the caller filled it */
int rvb_test_gather_pairs(const float* table, int rows, int64_t ld, const int32_t* row, const int32_t* col, int n, float* out);
int rvb_test_lse_gather_multi(const float* logits, int R, int V, const int32_t* ptr /* [R+1] */, const int32_t* target,
                              int P, float* out /* [P] */);
/* softmax_topk.hip row_xent on host logits [R][ld] (the first V entries of a row count): logp [ptr[R]] as rvb_test_lse_gather_multi,
 * and per row lse, sum_x (fp64) and top1.  Arguments are checked (RVB_E_ARG: ptr not ascending from 0, a target outside [0, V),
 * ld < V) before any device work. */
int rvb_test_row_xent(const float* logits, int R, int V, int ld, const int32_t* ptr /* [R+1] */, const int32_t* target,
                      float* logp /* [ptr[R]] */, float* lse /* [R] */, double* sum_x /* [R] */, int32_t* top1 /* [R] */);
/* host only: the trie of distinct hypothesis prefixes attention rescoring computes decoder rows for (trie.h build_trie_range, merge_tries) */
int rvb_test_build_trie(const int32_t* tokens, const int32_t* lens, const int32_t* chunk_of, int n_hyps, int n_chunks, int sos, int eos,
                        int reversed, int32_t* n_rows, int32_t* tok, int32_t* pos, int32_t* path, int32_t* hq_start, int32_t* hq_len,
                        int32_t* hq_pos0, int32_t* tgt_ptr, int32_t* tgt, int32_t* pair_slot, int32_t* n_work);
/* host only: the worker pool of the CTC search / trie building (engine.h HostPool) runs `rounds` jobs on up to n_threads threads;
 * fails unless every work item of every job was executed exactly once */
int rvb_test_host_pool(int n_threads, int items, int rounds);
/* ctc_viterbi.hip: forced alignment of tokens[L] over host log-probs lp [T][V] with the kernels rvb_ctc_align runs, advancing
 * slab_rows frames per launch (alpha carried in HBM between launches).  labels_out[T] = z[state] per frame, score_out = the fp32
 * path score.  Refuses (before any device work, by name): L = 0, ids outside [0, V) or equal to blank, a transcript T frames cannot
 * emit, sizes above the caps of include/rvb.h. */
int rvb_test_ctc_viterbi(const float* lp, int T, int V, const int32_t* tokens, int L, int blank, int slab_rows, int32_t* labels_out,
                         float* score_out);
/* the same with wildcards (the kernels rvb_ctc_align_wild runs): tokens may hold RVB_CTC_WILDCARD, which emits w[t] + bias at frame t
 * (w [T] host-supplied: the tests pass the row maxima of lp) and appears as RVB_CTC_WILDCARD in labels_out.  Refuses what
 * rvb_test_ctc_viterbi refuses, and a bias that is positive or not finite, before any device work; outputs untouched. */
int rvb_test_ctc_viterbi_wild(const float* lp, int T, int V, const float* w, float bias, const int32_t* tokens, int L, int blank,
                              int slab_rows, int32_t* labels_out, float* score_out);
/* ctc_viterbi_window.hip: the windowed kernels and the driver rvb_ctc_align_long_* runs, over host log-probs fed slab_rows frames at
 * a time (each slab cut into launches of at most W / 4 frames).  w == NULL: no wildcard (the plain kernels; RVB_CTC_WILDCARD is then
 * an id outside the vocabulary); w given: the WILD kernels, whether or not a token is a wildcard.  window_states: 0 or a multiple of 256 in [256, 32768], reduced to S rounded up to 32.  lo_out[T]:
 * the first state of each frame's window; min_margin_out: the path's smallest distance to a window edge that is not the lattice's
 * own (W when no frame counts).  Refuses before any device work, outputs untouched, what rvb_test_ctc_viterbi_wild refuses (no token
 * cap) and a bad window_states; a path that does not exist inside the windows is refused after the pass. */
int rvb_test_ctc_viterbi_window(const float* lp, int T, int V, const float* w, float bias, const int32_t* tokens, int L, int blank,
                                int slab_rows, int window_states, int32_t* labels_out, float* score_out, int32_t* lo_out,
                                int32_t* min_margin_out);
/* the host-only window policy (engine.h ctc_window_next_lo) */
int rvb_test_ctc_window_next_lo(int S, int T, int W, int f0, int f1, int lo_prev, int best_prev);
/* ctc_graph.hip: alignment of n_seq token graphs (arguments as rvb_ctc_align_graph) over host log-probs with the kernels
 * rvb_ctc_align_graph runs: lp is the lattices' frames concatenated ([sum T][V]), w [sum T] the wildcard's emission less the bias
 * (nullable when no node is a wildcard), slab_rows frames per launch (a slab may end inside a lattice or span several).
 * labels_out / frame_node_out [sum T]: the label (blank on a blank) and node (-1 on a blank) per frame; score_out [n_seq].  Refuses
 * what rvb_ctc_align_graph refuses, in the same words, before any device work; outputs untouched. */
int rvb_test_ctc_viterbi_graph(const float* lp, const int32_t* T, int n_seq, int V, const float* w, float bias, const int32_t* node_tokens,
                               const int32_t* n_nodes, const int32_t* pred_off, const int32_t* preds, const uint8_t* is_final, int blank,
                               int slab_rows, int32_t* labels_out, int32_t* frame_node_out, float* score_out);
/* ctc_graph_window.hip: the windowed graph kernels and the driver rvb_ctc_align_graph_long_* runs, for ONE graph (arguments as
 * rvb_ctc_align_graph_long_begin's) over host log-probs lp [T][V] fed slab_rows frames at a time; w [T] the wildcard's emission less
 * the bias (nullable when no node is a wildcard).  window_nodes: 0 or a multiple of 256 in [256, 8192], reduced to the nodes rounded
 * up to 64.  Without lo_force every slab is cut into launches by the policy (ctc_graph_window_next).  lo_force (nullable) replaces
 * the policy: every slab is then ONE launch, in the window lo_force[slab]; refused unless every entry is a multiple of 64 in
 * [0, max(0, N rounded up to 64 - W)], the entries do not decrease and entry 0 is 0.  labels_out / frame_node_out [T] as
 * rvb_test_ctc_viterbi_graph's; lo_out [T]: the first node of each frame's window; min_margin_out: the path's smallest distance to
 * a window edge that is not the graph's own (W when no frame counts); launches_out: kernel launches of the forward pass.  Refuses
 * what rvb_ctc_align_graph_long_begin refuses, in the same words, and a bad lo_force, before any device work; a band that holds no
 * path is refused (RVB_E_ARG) after the pass.  Outputs untouched on every refusal. */
int rvb_test_ctc_graph_window(const float* lp, int T, int V, const float* w, float bias, const int32_t* node_tokens, int n_nodes,
                              const int32_t* pred_off, const int32_t* preds, const uint8_t* is_final, int blank, int slab_rows, int window_nodes,
                              const int32_t* lo_force, int32_t* labels_out, int32_t* frame_node_out, float* score_out, int32_t* lo_out,
                              int32_t* min_margin_out, int32_t* launches_out);
/* the host-only window policy (engine.h ctc_graph_window_next) on a given graph (blank id 0): n_query launches, each described by its
 * first frame f0, its slab's end fend, the window before and the node the launch before reported (-1: none) -> its window and its
 * end.  Refuses what rvb_ctc_align_graph_long_begin refuses and a query outside the lattice.  No device work. */
int rvb_test_ctc_graph_window_next(const int32_t* node_tokens, int n_nodes, const int32_t* pred_off, const int32_t* preds,
                                   const uint8_t* is_final, int T, int V, int window_nodes, int n_query, const int32_t* f0,
                                   const int32_t* fend, const int32_t* lo_prev, const int32_t* best_prev, int32_t* lo_out, int32_t* f1_out);
/* ctc_forward_backward.hip: full-sum score of tokens[L] over host log-probs lp [T][V] with the kernels rvb_ctc_score runs, advancing
 * slab_rows frames per launch in both sweeps (forward ascending, backward descending from the last frame).  loglik_out is fp64; the
 * four per-token outputs [L] are nullable, and with all four null only the forward sweep runs.  Refuses what rvb_test_ctc_viterbi
 * refuses, in the same words.  RVB_CTC_SCORE_FAKE_NOMEM_ABOVE=<bytes> (lab switch) makes alpha rows above that size fail as an
 * allocation would: RVB_E_NOMEM naming the byte count, with nothing allocated. */
int rvb_test_ctc_score(const float* lp, int T, int V, const int32_t* tokens, int L, int blank, int slab_rows, double* loglik_out,
                       float* occupancy, float* mean_frame, float* peak_post, int32_t* peak_frame);
/* ctc_fb_window.hip: the windowed forward-backward kernels and the driver rvb_ctc_score_long_* runs, over host log-probs fed
 * slab_rows frames at a time (forward slabs ascending, backward slabs descending; each slab cut into launches as
 * rvb_test_ctc_viterbi_window's).  window_states as there.  lo_force (nullable, one entry per launch) replaces the policy's answer
 * launch by launch: refused unless every entry is a multiple of 32 in [0, S_pad - W], the entries do not decrease and entry 0 is 0.
 * lo_out [T]: the first state of each frame's window; best_out (nullable, one entry per launch): the state each launch reported.
 * The four per-token outputs are nullable, and with all four null only the forward sweep runs.  Refuses before any device work,
 * outputs untouched, what rvb_test_ctc_viterbi_window refuses (no wildcards), a bad lo_force and alpha rows (T x W x 4 bytes) above
 * RVB_CTC_SCORE_FAKE_NOMEM_ABOVE; a band that holds no path is refused after the forward pass. */
int rvb_test_ctc_score_window(const float* lp, int T, int V, const int32_t* tokens, int L, int blank, int slab_rows, int window_states,
                              const int32_t* lo_force, double* loglik_out, float* occupancy, float* mean_frame, float* peak_post,
                              int32_t* peak_frame, int32_t* lo_out, int32_t* best_out);
/* the same for n_seq lattices in ONE launch per slab: lp is the lattices' frames concatenated ([sum T][V]), tokens their tokens
 * concatenated; outputs are concatenated alike.  A slab of slab_rows rows may end inside a lattice or span several. */
int rvb_test_ctc_score_batch(const float* lp, const int32_t* T, int V, const int32_t* tokens, const int32_t* L, int n_seq, int blank,
                             int slab_rows, double* loglik_out, float* occupancy, float* mean_frame, float* peak_post,
                             int32_t* peak_frame);
/* ctc_graph_score.hip: full-sum score of n_seq token graphs (arguments as rvb_ctc_score_graph) over host log-probs with the kernels
 * and the driver rvb_ctc_score_graph runs: lp is the lattices' frames concatenated ([sum T][V]), slab_rows frames per launch in both
 * sweeps.  loglik_out [n_seq] is fp64; the five per-node outputs are nullable and concatenated like node_tokens, and with all five
 * null only the forward sweep runs.  Refuses what rvb_ctc_score_graph refuses, in the same words, before any device work; outputs
 * untouched. */
int rvb_test_ctc_score_graph(const float* lp, const int32_t* T, int n_seq, int V, const int32_t* node_tokens, const int32_t* n_nodes,
                             const int32_t* pred_off, const int32_t* preds, const uint8_t* is_final, int blank, int slab_rows,
                             double* loglik_out, float* visit, float* occupancy, float* mean_frame, float* peak_post, int32_t* peak_frame);
/* ctc_graph_fb_window.hip: the windowed graph full-sum kernels and the driver rvb_ctc_score_graph_long_* runs, for ONE graph (arguments
 * as rvb_ctc_score_graph_long_begin's) over host log-probs lp [T][V] fed slab_rows frames at a time (forward slabs ascending, backward
 * slabs descending).  window_nodes: 0 or a multiple of 256 in [256, 4096], reduced to the nodes rounded up to 64.  Without lo_force
 * every slab is cut into launches by the policy (ctc_graph_window_next) from the best node each launch reports.  lo_force (nullable)
 * replaces the policy as in rvb_test_ctc_graph_window: every slab is then ONE launch, in the window lo_force[slab]; refused unless
 * every entry is a multiple of 64 in [0, max(0, N rounded up to 64 - W)], the entries do not decrease and entry 0 is 0.  loglik_out is
 * fp64; the five per-node outputs [n_nodes] are nullable, and with all five null only the forward sweep runs.  lo_out [T]: the first
 * node of each frame's window; best_out (nullable, one entry per launch, at most T): the node each forward launch reported;
 * launches_out (nullable): forward launches.  Refuses before any device work what rvb_ctc_score_graph_long_begin refuses, in the same
 * words, and a bad lo_force; a band that holds no path is refused (RVB_E_ARG) after the forward pass.  Outputs untouched on every
 * refusal. */
int rvb_test_ctc_score_graph_window(const float* lp, int T, int V, const int32_t* node_tokens, int n_nodes, const int32_t* pred_off,
                                    const int32_t* preds, const uint8_t* is_final, int blank, int slab_rows, int window_nodes,
                                    const int32_t* lo_force, double* loglik_out, float* visit, float* occupancy, float* mean_frame,
                                    float* peak_post, int32_t* peak_frame, int32_t* lo_out, int32_t* best_out, int32_t* launches_out);
/* ctc_find.hip: phrase search over host log-probs with exactly the kernel and the host code rvb_ctc_find runs.  lp holds the frames
 * of n_seq sequences concatenated ([sum T][V]; T[i] >= 0), w [sum T] each row's maximum (null: computed on the host from lp);
 * n_phrases phrases concatenated in `tokens`; threshold [n_phrases]; slab_rows rows per launch (h, st and the counts carried in HBM).
 * Pair p * n_seq + i.  RAW candidates as the kernel wrote them: raw_count [pairs] (all arrivals at or above the threshold),
 * raw_end / raw_start / raw_score [pairs][max_candidates] (the first min(count, max_candidates) slots of a pair are written);
 * hits after suppression: n_hits [pairs], hit_start / hit_end / hit_score [pairs][max_hits].  Refuses what rvb_ctc_find refuses, in
 * the same words, and a row maximum that is not finite, before any device work; outputs untouched. */
int rvb_test_ctc_find(const float* lp, const int32_t* T, int n_seq, int V, const float* w, const int32_t* tokens, const int32_t* tok_lens,
                      int n_phrases, const float* threshold, int blank, int slab_rows, int max_candidates, int max_hits,
                      int64_t* raw_count, int32_t* raw_end, int32_t* raw_start, float* raw_score, int32_t* n_hits, int32_t* hit_start,
                      int32_t* hit_end, float* hit_score);
/* host only, no device: the slab feed the four drivers above share (ctc_slabs.h) over plain descriptors.  rows: the row lists of
 * n_seq sequences back to back, T[i] >= 0 of them each, taken as a plan() takes them; slabs [n_slabs][2] = (r0, nrows), fed in the
 * order given: the ascending step from f0 = f1 = 0 or, with descending != 0, the backward step from f0 = f1 = T; then the sweep's
 * coverage check.  `who` is the prefix of the messages ("ctc align", ...).  Per slab fed: touches_out / any_out [n_slabs] and
 * windows_out [n_slabs][n_seq][2] = every sequence's (f0, f1) after it.  fed_out: the slabs fed before a refusal; covered_out: 1 when
 * the coverage check passed.  Returns the first refusal (rvb_last_error), RVB_OK when there was none. */
int rvb_test_slab_windows(const char* who, const int32_t* rows, const int32_t* T, int n_seq, const int32_t* slabs, int n_slabs,
                          int descending, int32_t* windows_out, int32_t* any_out, int32_t* touches_out, int32_t* fed_out,
                          int32_t* covered_out);
int rvb_test_fbank(const int16_t* pcm, int64_t n_samples, float* feats /* [frames,80] */);
/* fbank (pcm non-null) or fbank_f32 (wave non-null: a float waveform at int16 scale, as the resampler leaves it) with the engine's
 * tables; exactly one of the two is given.  The device waveform holds exactly n_samples elements.  feats [frames + 4][80]: the device
 * buffer starts as all-ones bytes and comes back whole, so the four rows after the last frame show whether anything was written
 * past it (n_samples < 400: no frame, no launch, four sentinel rows). */
int rvb_test_fbank_ex(const int16_t* pcm, const float* wave, int64_t n_samples, float* feats /* [frames + 4][80] */);
/* fbank_batch (the segmented kernel behind rvb_fbank_batch, with its memset) on caller-given recordings: data[r] holds n_samples[r]
 * int16 (sample_format RVB_SAMPLE_I16) or float (RVB_SAMPLE_F32) samples at 16 kHz, placed at element offset[r] of the packed device
 * buffer of its format (NULL: packed back to back; each buffer is allocated to exactly the last sample any recording covers).  feats
 * [total_chunks * chunk_size + 4][80] in the layout of rvb_batch_plan; the four rows behind the last chunk are sentinels (all-ones
 * bytes) that the launch must leave alone.  Overlapping or negative offsets are refused (RVB_E_ARG) before any device work. */
int rvb_test_fbank_batch(const void* const* data, const int32_t* sample_format, const int64_t* n_samples, const int64_t* offset, int n_rec,
                         int chunk_size, float* feats);
/* native prefix beam search on host arrays: top-k log-probs/indices [T,beam] of one utterance */
int rvb_test_prefix_beam(const float* topk_val, const int32_t* topk_idx, int T, int beam, int blank,
                         int32_t* n_hyps, int32_t* tokens /* [beam][T] */, int32_t* lens, int32_t* times,
                         int32_t* times_lens, double* scores);
/* the same search with a hot-word context graph (search.cpp ContextGraph; host only).  The phrases go through the checks of
 * rvb_set_context_graph against `vocab` and `blank` first (RVB_E_ARG by name).  n_phrases < 0: no graph at all; 0: a graph of the
 * root alone.  scores = score + context score; context_scores (nullable) = the context score each hypothesis ends with. */
int rvb_test_prefix_beam_context(const float* topk_val, const int32_t* topk_idx, int T, int beam, int blank, int vocab,
                                 const int32_t* phrase_tokens, const int32_t* phrase_lens, int n_phrases, double context_score,
                                 int32_t* n_hyps, int32_t* tokens /* [beam][T] */, int32_t* lens, int32_t* times, int32_t* times_lens,
                                 double* scores, double* context_scores);
/* the graph alone: from the root, forward_one_step over stream[n_steps]; per step the score and the node id reached, and what
 * finalize returns from that node.  num_nodes (nullable) = nodes below the root. */
int rvb_test_context_walk(const int32_t* phrase_tokens, const int32_t* phrase_lens, int n_phrases, double context_score, int vocab,
                          int blank, const int32_t* stream, int n_steps, int32_t* num_nodes, double* step_scores, int32_t* step_nodes,
                          double* final_scores);

/* diarization kernels (diar.hip, resnet.hip tstp_pool) on host floats; see test_api.hip for the layouts */
int rvb_test_window_stats(const float* wave, int64_t n, int64_t first, int nwin, int64_t step, int len, float eps, float* stats);
int rvb_test_sinc_conv(int dtype, const float* wave, int64_t n_samples, const float* filt, int nf, int ksize, int stride,
                       int64_t n_frames, float* out);
int rvb_test_pool_norm(int dtype, int first_block, const float* x, int rows_in, int ld_in, int frames_in, int C, int ld_out,
                       const float* gamma, const float* beta, float eps, int W, const float* craw, int64_t craw_rows,
                       int64_t craw_frame0, int craw_frames_per_step, const float* stats, const float* fsum, float wn_gamma,
                       float wn_beta, float* out);
int rvb_test_conv1d5(int cin, const float* A, int64_t rows, const float* W, const float* bias, float* out, int64_t M);
int rvb_test_lstm_layer(int dtype, const float* x, int W, int T, int in, const float* w_ih, const float* w_hh, const float* b_ih,
                        const float* b_hh, float* out);
int rvb_test_classifier(int dtype, const float* x, int ldx, const float* w, const float* b, float* logp, uint8_t* cls,
                        int64_t M, int in, int C);
int rvb_test_tstp(int dtype, const float* x, int B, const int32_t* item_b, const float* mask, int mask_len, int n_items, int F,
                  int TT, int C, float* stats);
/* embedding trunk (resnet.hip, conv_gemm.hip, conv_row64.hip, conv_stream.hip) on host floats; see test_api.hip for the layouts.
 * conv2d: one convolution through a named path (0 = conv2d's dispatch, 1 = direct, 2 = implicit GEMM, 3 = row64, 4 = stream),
 * optionally with the fused projection shortcut (x2 / w2); ran[2] = {kernel that ran, its tile}.  emb_stem: emb_window_mean over
 * all windows, then emb_conv1 on the listed ones. */
int rvb_test_conv2d(int dtype, int path, const float* x, const float* w, const float* bias, const float* res, float* out, int B, int Fi,
                    int Ti, int Cin, int Cout, int stride, int taps, int relu, const float* x2, const float* w2, int Fi2, int Ti2, int Cin2,
                    int stride2, int32_t* ran);
int rvb_test_emb_stem(int dtype, const float* fb, int64_t n_rows, const int64_t* win, int B, int n_windows, int frames_per_step, int nfr,
                      int F, int C, const float* w, const float* bias, float* mean, float* out);
/* clustering (linkage.hip).  pdist_nn: the two launches centroid_linkage() starts with, on host X [n][d] (n >= 2): the device D [n][n],
 * neighbor [n] and min_dist [n] start as all-ones bytes and come back whole, so an element no kernel wrote comes back NaN / -1 (slot
 * n - 1 of neighbor and min_dist always does: nn_init's grid is n - 1).
 * centroid_linkage: centroid_linkage() on the allocations, the initial state and the 4096-byte control block rvd_centroid_linkage
 * makes, then its status check and its slot-to-id conversion: Z [n-1][4] as scipy.cluster.hierarchy.linkage(X, "centroid") lays it
 * out, written only on success.  workgroups as rvd_set_linkage_workgroups takes it.  ran[4] = {loop, G, exchange form, fell_back}:
 * loop 1 = LDS state + slot compaction, 2 = LDS state, 3 = state in global memory, 4 = multi-workgroup; G = workgroups of the loop
 * (1 for loops 1-3); exchange form 0 = A, 1 = B, 2 = C (0 for loops 1-3); fell_back = 1 when the multi-workgroup loop gave up and
 * the one-workgroup loop produced Z.  retries (nullable) = stale candidates the loop re-evaluated (workgroup 0's, in loop 4).
 * Refuses what rvd_centroid_linkage refuses (n < 1, d < 1, n > 46000, no candidate pair) in its words.  The lab switches
 * RVD_LINKAGE_MB / _G / _XCHG / _COMPACT / _GLOBAL apply. */
int rvb_test_pdist_nn(const double* X, int n, int d, double* D /* [n][n] */, int32_t* neighbor /* [n] */, double* min_dist /* [n] */);
int rvb_test_centroid_linkage(const double* X, int n, int d, int workgroups, double* Z /* [n-1][4] */, int32_t* ran /* [4] */,
                              double* retries);
/* rvd_centroid_linkage_many without an engine: X [sum n][d] and Z [sum max(n-1,0)][4], problems back to back.  route[p]: 1 or 2 =
 * the batched one-workgroup loop that ran (2 under RVD_LINKAGE_COMPACT=0), 0 = routed to the single call (3 000 points or more, or
 * RVD_LINKAGE_GLOBAL), -1 = fewer than 2 points, nothing to do.  A problem without a candidate pair fails the call, its index in
 * the message. */
int rvb_test_centroid_linkage_many(const double* X, const int32_t* n, int n_problems, int d, double* Z, int32_t* route);

/* GEMM kernel selection / micro-benchmark hooks (tests and tuning only) */
int rvb_test_set_gemm_variant(int variant /* 0 auto, 1 gemm.hip 128x128, 2 gemm2.hip 256x256 LDS-DMA */);
/* gemm2.hip tuning switches: flags bit 0 = 32x32x16 MFMAs, bit 1 = s_setprio for the later-dispatched waves;
 * group_m = tile order (0/1 row-major inside an XCD's run, n = n row tiles down then the next column); -1 = defaults */
int rvb_test_set_gemm2_opts(int flags, int group_m);
/* per-workgroup phase timestamps of one bf16 gemm2 launch (measurement aid, scripts/gemm_timeline.py) */
int rvb_test_gemm_timeline(int M, int N, int K, int act, int out_f32, int with_res, long long* out, int cap, int* n_wg);
int rvb_test_gemm_bench(int dtype, int M, int N, int K, int variant, int iters, int act, int out_f32, int with_res,
                        double* ms_out, double* max_abs_diff_vs_variant1);

/* pause_chunks.hip: the loudness and cut-search kernels behind rvb_pause_chunks on host feature rows feats [n_rows][80]: recording r
 * owns the rows [row0[r], row0[r] + n_frames[r]); the rows between recordings may hold anything.  starts: every recording's piece
 * starts, concatenated in recording order (at most `capacity` entries: RVB_E_ARG naming the count if more); counts [n_rec].  The
 * parameters are refused as by rvb_pause_chunks, before any device work, in this hook's name. */
int rvb_test_pause_cuts(const float* feats, int64_t n_rows, const int64_t* row0, const int64_t* n_frames, int n_rec, int chunk_size,
                        int search, int h, int32_t* starts, int64_t capacity, int32_t* counts);
/* pause_chunks.hip: the gather kernel alone: lens[k] rows from row src[k] of feats [n_rows][80] to rows [k * chunk_size ..) of out
 * [n_pieces * chunk_size + 1][80], the rest of each slot zero; the device buffer starts as all-ones bytes and comes back whole, so
 * the row behind the last slot shows whether anything was written past it. */
int rvb_test_gather_chunks(const float* feats, int64_t n_rows, const int64_t* src, const int32_t* lens, int64_t n_pieces,
                           int chunk_size, float* out);

#ifdef __cplusplus
}
#endif
#endif /* RVB_TEST_API_H_ */
