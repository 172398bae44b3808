// What the engine's translation units share: engine.hip (error text, buffers, profiling, uploads, the GEMM / norm wrappers and the C ABI),
// engine_weights.hip, engine_encode.hip, engine_decode.hip, engine_ctc.hip.  test_api.hip reads it for make_fbank_tables.  Internal:
// everything is in namespace rvb and nothing has C linkage; what one file alone needs stays static in that file.
#pragma once
#include "engine.h"

namespace rvb {

// ---- engine.hip
// the profiling bracket of one stage: counts the launch, and with profiling on times it between two events on the engine's stream
struct Scope {
  rvb_engine* e; hipEvent_t a = nullptr, b = nullptr; std::string name;
  Scope(rvb_engine* e_, const char* n, double flops = 0.0, double bytes = 0.0) : e(e_), name(n) {
    auto& pe = e->prof[name];
    pe.launches += 1; pe.flops += flops; pe.bytes += bytes;
    if (e->profiling == 0 || (e->profiling == 2 && name != "gemm" && name != "gemm_fp8")) return;
    auto get = [&]() { hipEvent_t ev; if (!e->event_pool.empty()) { ev = e->event_pool.back(); e->event_pool.pop_back(); } else (void)hipEventCreate(&ev); return ev; };
    a = get(); b = get();
    (void)hipEventRecord(a, e->stream);
  }
  ~Scope() {
    if (!a) return;
    (void)hipEventRecord(b, e->stream);
    e->pending.push_back({a, b, name});
  }
};
int upload_f32(rvb_engine* e, DevBuf& dst, const float* src, size_t n);
int upload_i32(rvb_engine* e, DevBuf& dst, const int32_t* src, size_t n);
const AttnArgs& with_lab(AttnArgs& a);
int reset_f8sat(rvb_engine* e);
double gemm_alg_bytes(const rvb_engine* e, const GemmArgs& g);
int run_gemm(rvb_engine* e, const void* A, int lda, const Linear& L, void* C, int ldc, int M, bool out_f32,
             float alpha = 1.f, int act = ACT_NONE, const float* res = nullptr, int ldres = 0);
int run_norm(rvb_engine* e, const float* x, const LNorm& n, void* out, bool out_f32, int M, int d,
             int mode = NORM_LN, int silu = 0, const void* add = nullptr, const LNorm* second = nullptr,
             void* out2 = nullptr, float out8 = 0.f, float out2_8 = 0.f, bool x_bf16 = false, unsigned* sat = nullptr,
             unsigned* sat2 = nullptr);
int run_gemm8(rvb_engine* e, const void* A8, int lda, const Linear& L, void* C, int ldc, int M, float a_scale, int out_kind,
              float out_scale = 1.f, float alpha = 1.f, int act = ACT_NONE, const float* res = nullptr, int ldres = 0,
              unsigned* sat = nullptr);

// encoder taps (rvb_set_encoder_tap): both do nothing unless rvb_encode is inside the tapped position (e->tap_live)
int tap_keep(rvb_engine* e, const char* name, const void* src, size_t elems, bool is_bf16);     // device-to-device copy on the engine's stream
void tap_note_gemm(rvb_engine* e);       // after a gemm() call: appends which kernel file it chose (gemm_last_path)
int gemm_last_path();                    // gemm.hip: 2 = gemm2.hip, 1 = gemm.hip -- what gemm() dispatched to last on this thread
void tap_note_attention(rvb_engine* e);  // after an attention() call: appends the eight integers of attention_last_form

// ---- engine_weights.hip
int make_fbank_tables(rvb_engine* e);
int finalize_impl(rvb_engine* e, const float* cat, int ncat);
int set_fp8_policy_impl(rvb_engine* e, int groups, int first_block, int last_block);

// ---- engine_encode.hip
constexpr int LOGIT_SLAB = 8192;   // rows of fp32 logits materialised at a time
int wait_slices(rvb_engine* e, int i);
int encode_impl(rvb_engine* e, const float* feats, int64_t first_chunk, const int32_t* lens, int B, int T0, int beam, float blank_penalty);
int stream_begin_impl(rvb_engine* e);
int stream_chunk_impl(rvb_engine* e, const float* feats, int T0, int required_cache_size, float* out, int32_t* n_out);
int stream_finish_impl(rvb_engine* e, int beam, float blank_penalty);

// ---- engine_decode.hip
int prefix_beam_impl(rvb_engine* e, int beam);
int decoder_memory_kv(rvb_engine* e, Decoder& D, int M);
int rescore_impl(rvb_engine* e, double ctc_weight, double reverse_weight);
int attention_decode_impl(rvb_engine* e, int N, float length_penalty);
int joint_decode_impl(rvb_engine* e, int beam, double ctc_weight, double pre_beam_ratio, double length_bonus);

}  // namespace rvb
