// Host-side entry points of the CDNA4 kernel library (implemented in *.hip).
#pragma once

#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <cstdint>

namespace tepdist {

using bf16 = __hip_bfloat16;

// --- GEMM ------------------------------------------------------------------
// C[M,N] = A @ B (+bias, +gelu epilogue). Layout flags:
//   a_kc: A stored row-major [M,K] (k-contiguous); else stored [K,M].
//   b_kc: B stored row-major [N,K] (k-contiguous, i.e. the operand is a
//         transposed weight W[N,K]); else stored [K,N].
// epi (the EPI_* enum of gemm_plan.h): 0 = none, 1 = +bias, 2 = +bias+gelu
//      (writes pre-act to c_pre), 3 = gelu only (writes pre-act to c_pre),
//      4 = dgelu: C = (A @ B) * gelu'(c_pre), c_pre being the INPUT
//      pre-activation saved by the forward.
// Batched over `batch` with element strides; stride 0 broadcasts.
// gemm_plan() (gemm_plan.h) decides the kernel and the K split from the
// arguments alone; gemm_bf16 launches that plan and throws with the plan's
// reason when no kernel accepts the call (epi 4 outside the 256 kernel's
// case). When the plan splits K (split_k > 1), splitk_ws must hold
// split_k * M * N floats and ldc must be N: the chunks write fp32 partials
// there and a second launch reduces them into C. splitk_ws may be null
// otherwise.
// colsum_out (bf16 [M], may be null): also returns A's column sums,
// colsum[m] = sum over k of A[k][m] (wgrad's bias gradient), formed by the
// 256 kernel from the fragments it holds anyway. Only for a 256-kernel plan
// on two k-outer operands (colsum_why_not, gemm_plan.h), else it throws.
// The workspace then holds gemm_ws_floats(plan, M, N, true) floats, split
// or not; no part of it needs zeroing and no atomics run, so the sums are
// the same bits on every call.
void gemm_bf16(const void* A, const void* B, void* C, void* c_pre,
               const void* bias, int M, int N, int K, int lda, int ldb,
               int ldc, int64_t stride_a, int64_t stride_b, int64_t stride_c,
               int batch, bool a_kc, bool b_kc, int epi, float* splitk_ws,
               void* colsum_out, hipStream_t stream);
// Launcher of the deep-pipelined 256x256 kernel, for gemm_bf16 only: runs
// the plan it is given (split_k > 1: C is the fp32 workspace). k_outer:
// both operands stored [K][F] (a_kc = b_kc = false), epi 0 only.
// colsum_parts (k_outer, batch 1; else null): fp32 column-sum parts of A,
// split_k * (N/256) vectors of M floats, for gemm_bf16's reduce.
void gemm256_bf16(const void* A, const void* B, void* C, void* c_pre,
                  const void* bias, int M, int N, int K, int lda, int ldb,
                  int ldc, int64_t stride_a, int64_t stride_b,
                  int64_t stride_c, int batch, bool k_outer, int epi,
                  int split_k, int k_chunk, float* colsum_parts,
                  hipStream_t stream);

// --- Transpose -------------------------------------------------------------
// out[c][r] = in[r][c] per batch (strides in elements).
void transpose_bf16(const void* in, void* out, int R, int C,
                    int64_t stride_in, int64_t stride_out, int batch,
                    hipStream_t stream);
void cast_ws_f32_bf16(const float* ws, void* db_out, int cols,
                      hipStream_t stream);
void transpose_dy_bf16(const void* dy, const void* pre, void* dy_t,
                       void* dy_nat, float* bias_ws, int R, int C,
                       hipStream_t stream);

// --- LayerNorm -------------------------------------------------------------
// res/sum_out non-null = fused residual add: sum_out := x + res (rounded
// once to bf16), statistics and y over the sum. dsum non-null in bwd adds
// the straight-through gradient into dx in the same pass.
void layernorm_fwd_bf16(const void* x, const void* gamma, const void* beta,
                        void* y, float* mean, float* rstd, int rows, int cols,
                        float eps, hipStream_t stream,
                        const void* res = nullptr, void* sum_out = nullptr);
void layernorm_bwd_bf16(const void* dy, const void* x, const void* gamma,
                        const float* mean, const float* rstd, void* dx,
                        float* dgamma_part, float* dbeta_part, int rows,
                        int cols, int part_rows, hipStream_t stream,
                        const void* dsum = nullptr);
void layernorm_bwd_reduce(const float* dgamma_part, const float* dbeta_part,
                          void* dgamma, void* dbeta, int part_rows, int cols,
                          hipStream_t stream);

// --- Softmax (fused scale + causal mask) -----------------------------------
// x: [rows, cols] rows = B*H*Sq, cols = Sk; causal masks col > row_in_tile
// (with q_offset = Sk - Sq so the last query attends to everything).
void softmax_fwd_bf16(const void* x, void* p, int64_t rows, int cols, int sq,
                      float scale, bool causal, hipStream_t stream);
void softmax_bwd_bf16(const void* dp, const void* p, void* ds, int64_t rows,
                      int cols, float scale, hipStream_t stream);

// --- Fused flash attention (causal) ---------------------------------------
// Strided [B, H, S, D] addressing (D contiguous): q/k/v share
// (q_bs, q_hs, q_rs) batch/head/row strides — a packed [B,S,3d] qkv is
// three base pointers with the same strides; o/dout use (o_bs, o_hs, o_rs).
// lse/delta: [B*H, S] f32; dq_ws: zeroed f32 [B*H, S, D] accumulated with
// atomics (cast/scattered by the caller).
void attention_fwd_bf16(const void* q, const void* k, const void* v, void* o,
                        float* lse, int B, int H, int S, int D, float scale,
                        bool causal, int64_t q_bs, int64_t q_hs, int64_t q_rs,
                        int64_t o_bs, int64_t o_hs, int64_t o_rs,
                        hipStream_t stream);
void attention_bwd_bf16(const void* q, const void* k, const void* v,
                        const void* o, const void* dout, const float* lse,
                        float* delta, void* dq, void* dk, void* dv,
                        int B, int H, int S, int D, float scale, bool causal,
                        int64_t q_bs, int64_t q_hs, int64_t q_rs,
                        int64_t o_bs, int64_t o_hs, int64_t o_rs,
                        hipStream_t stream);

// --- Decode attention (single query over a KV cache) ----------------------
// q/k_new/v_new: [B,H,D] bf16, D contiguous, (bs, hs) element strides
// (q_* for q, n_* shared by k_new/v_new; both may be null). k/v_cache:
// [B,H,S_max,D] bf16 sharing (c_bs, c_hs, c_rs). pos: device int64, read
// at pos[b * pos_stride] (pos_stride 0 or 1) and clamped into
// [0, S_max-1] in the kernel. Without new rows the query attends cache
// rows 0..p; with them it attends rows 0..p-1 plus the new row, which is
// also stored into cache[b,:,p,:] (equal to write-then-attend; cache row p
// is never read by that launch). out: [B,H,D] bf16 contiguous. ws: fp32
// [B*H*splits*(D+2)], only read when splits > 1. D in {64,128},
// splits in [1,32]; anything else throws.
// Grouped-query attention: the caches and k_new/v_new hold Hkv heads, q and
// out hold H = G*Hkv with G in {1,2,4,8}; query head h attends K/V head
// h / G. With rope, q and k_new are rotated (rotate-half, theta =
// rope_theta) by the clamped position p inside the kernel: q in fp32,
// k_new rounded to bf16 once, attended to and stored in that form (the
// cache holds rotated rows); v_new is stored as is.
void decode_attention_bf16(const void* q, const void* k_new,
                           const void* v_new, void* k_cache, void* v_cache,
                           const int64_t* pos, int pos_stride, void* out,
                           float* ws, int B, int H, int Hkv, int S_max,
                           int D, float scale, int splits, bool rope,
                           float rope_theta, int64_t q_bs,
                           int64_t q_hs, int64_t n_bs, int64_t n_hs,
                           int64_t c_bs, int64_t c_hs, int64_t c_rs,
                           hipStream_t stream);

// --- Token sampling (sampling.hip) -----------------------------------------
// out[b] (int64 [B]) := one token of row b of logits [B, >= vocab] (fp32, or
// bf16 when logits_bf16; columns contiguous, rows row_stride elements
// apart, any alignment), drawn from softmax(z / temperature) over columns
// < vocab after top-k (0 or >= vocab: off; ties at the k-th value kept) and
// top-p (>= 1: off) by inverse CDF in index order. The uniform is u[b]
// (fp32) or, when u is null, the first word of Philox4(seed, b, step[0]);
// exactly one of u and step is given. tau (fp32 [B], may be null) receives
// the final threshold: columns with z >= tau were kept. Always
// 0 <= out[b] < vocab. One workgroup per row, no workspace, no host sync;
// vocab <= 2^22 keeps every 64-bit sum of the 2^40-scaled weights below
// 2^62; temperature <= 0, top_p <= 0 or vocab > 2^22 throws.
void sample_logits(const void* logits, bool logits_bf16, int64_t row_stride,
                   int B, int vocab, float temperature, int top_k,
                   float top_p, uint64_t seed, const int64_t* step,
                   const float* u, int64_t* out, float* tau,
                   hipStream_t stream);

// --- MoE routing / dispatch / combine (moe_route.hip) ----------------------
// All maps are int32. gates [T,E] contiguous (bf16, or fp32 when
// gates_fp32), 2 <= E <= 64, 1 <= k <= min(4,E), C >= 1, T*k < 2^31,
// E*C < 2^31. Writes every element of topi [T,k] (k largest gates, ties to
// the lower expert), slot [T,k] (e*C + pos in stable flat order, -1 when
// pos >= C), src [E*C] (t*k + j of the entry in the slot, -1 when empty)
// and counts [E] (selections per expert before dropping). ws: int32
// [moe_route_ws_ints(T, E)], overwritten. Three launches, no atomics.
int64_t moe_route_ws_ints(int T, int E);
void moe_route(const void* gates, bool gates_fp32, int* topi, int* slot,
               int* src, int* counts, int* ws, int T, int E, int k, int C,
               hipStream_t stream);
// out [EC,d] := (w[src[s]] *) in[src[s] / k, :] for a filled slot, zeros for
// an empty one; in [T,d]. w null = unweighted (dispatch fwd); w fp32 [T*k]
// = combine bwd dy. bf16 rows, d % 8 == 0, 16-byte aligned bases,
// EC * d / 8 < 2^31.
void moe_gather_rows_bf16(const void* in, const int* src, const float* w,
                          void* out, int T, int k, int64_t EC, int d,
                          hipStream_t stream);
// out [T,d] := sum over kept j of (w[t,j] *) in[slot[t,j], :]; in [EC,d];
// fp32 accumulation, one rounding. w null = dispatch bwd, else combine fwd.
void moe_reduce_rows_bf16(const void* in, const int* slot, const float* w,
                          void* out, int T, int k, int64_t EC, int d,
                          hipStream_t stream);
// dw [T,k] fp32 := dot(y[slot[t,j], :], dout[t, :]), exactly 0 when dropped.
void moe_combine_dw_bf16(const void* y, const void* dout, const int* slot,
                         float* dw, int T, int k, int64_t EC, int d,
                         hipStream_t stream);

// --- Embedding -------------------------------------------------------------
void embedding_fwd_bf16(const int64_t* ids, const void* table, void* out,
                        int64_t n_ids, int dim, hipStream_t stream);
void embedding_bwd_bf16(const void* dy, const int64_t* ids, float* grad_f32,
                        void* grad_bf16, int64_t n_ids, int vocab, int dim,
                        hipStream_t stream);

// --- Cross entropy ---------------------------------------------------------
void cross_entropy_fwd_bf16(const void* logits, const int64_t* targets,
                            float* nll, float* lse, int64_t rows, int cols,
                            int ignore_index, hipStream_t stream);
void cross_entropy_bwd_bf16(const void* logits, const int64_t* targets,
                            const float* lse, const float* dscale,
                            void* dlogits, int64_t rows, int cols,
                            int ignore_index, hipStream_t stream);

// --- Dropout ---------------------------------------------------------------
void dropout_fwd_bf16(const void* x, void* y, uint8_t* mask, int64_t n,
                      float p, uint64_t seed, uint64_t offset,
                      hipStream_t stream);
void dropout_bwd_bf16(const void* dy, const uint8_t* mask, void* dx, int64_t n,
                      float p, hipStream_t stream);

// --- Elementwise -----------------------------------------------------------
void gelu_fwd_bf16(const void* x, void* y, int64_t n, hipStream_t stream);
void gelu_bwd_bf16(const void* dy, const void* x, void* dx, int64_t n,
                   hipStream_t stream);
void bias_sum_bf16(const void* dy, void* db, float* ws_zeroed, int64_t rows,
                   int cols, hipStream_t stream);

// --- AdamW fused step ------------------------------------------------------
void adamw_bf16(void* param, float* master, const void* grad_bf16,
                const float* grad_f32, float* exp_avg, float* exp_avg_sq,
                int64_t n, float lr, float beta1, float beta2, float eps,
                float weight_decay, float bc1, float bc2, hipStream_t stream);

// multi-tensor fused AdamW (pointer tables on device; MT_CHUNK=16384)
void adamw_mt_bf16(const int64_t* tabs, const int64_t* numel,
                   const float* wds, const unsigned char* ptypes,
                   const int* chunks, int nchunks, int nt,
                   float lr, float beta1, float beta2, float eps, float bc1,
                   float bc2, const float* hyper, hipStream_t stream);

// --- diagnostics -----------------------------------------------------------
void tr16_probe(float* out_pattern, float* out_uniform, hipStream_t stream);
// out: int32 [2][C/16][64][8], see debug.hip
void tr16_frag_probe(int* out, int C, hipStream_t stream);

// --- Llama-family ops ------------------------------------------------------
void rmsnorm_fwd_bf16(const void* x, const void* g, void* y, float* rstd,
                      int64_t rows, int cols, float eps, hipStream_t stream);
void rmsnorm_bwd_bf16(const void* dy, const void* x, const void* g,
                      const float* rstd, void* dx, void* dgamma,
                      float* dg_part, int part_rows, int64_t rows, int cols,
                      hipStream_t stream);
void rope_bf16(const void* x, void* y, int64_t tokens, int heads, int D,
               int seq_len, float theta, bool backward, hipStream_t stream);
void swiglu_fwd_bf16(const void* a, const void* b, void* y, int64_t n,
                     hipStream_t stream);
void swiglu_bwd_bf16(const void* dy, const void* a, const void* b, void* da,
                     void* db, int64_t n, hipStream_t stream);

}  // namespace tepdist
