// ppo_fused.hpp — parameter block and host entry points of the fused PPO kernels (ppo_fused.hip), shared with ppo_engine.hip.
#pragma once
#include <hip/hip_runtime.h>

namespace mi {

struct PpoFusedParams {
    // flat parameter buffers (engine layout, offsets in floats) and optimiser state
    float *theta, *adam_m, *adam_v, *grads; const float* theta_old;
    long long off[13];
    int kin, din, H1, H2, A, M;
    long long n_params;                                   // floats in each flat buffer
    // activations (workspace): [net][M][H] with net 0 = policy, 1 = value, 2 = old policy
    const float *states, *actions, *returns, *adv, *low, *high;
    float *h1, *h2, *dh1, *dh2;                           // h1/h2: 3 nets; dh1/dh2: 2 nets
    float *du, *dv, *partial, *losses, *mean_out;
    // minibatch gather fused into the step (mi_ppo_train_step_idx): sample m of the minibatch is row row_idx[m] of the horizon-batch tables
    // states / actions / returns / adv / logp_old (n_rows rows each); layer 1 also leaves the gathered states in s_gath [M, din] for the filter gradient
    const int* row_idx; int n_rows;
    // wide inputs (mi_ppo_set_wide_inputs), in the 4 bytes of padding behind n_rows, so that no field moves and no kernel's argument offsets change.  The engine's
    // mode -- 0: the fused range ends at kin = 96; 1 / 2: at kin = 1024, and layer 1 of kin > 96 runs as ppo_l1_wide_kernel (1) or as ppo_l1_kernel (2)
    int wide;
    float* s_gath;
    const float* logp_old;                                // cached log pi_old(a|s) per sample (nullptr: recomputed from net 2)
    float* logp_out;                                      // when set: the loss kernel also stores log pi(a|s) (used to fill the cache)
    int n_nets;                                           // 3, or 2 with the cache
    float clip_eps, value_scale, entropy_scale, inv_m, grad_scale;
    float alpha, omb1, omb2, epsilon;                     // Adam: alpha = lr * sqrt(1 - b2^t) / (1 - b1^t); omb = 1 - beta
    int n_loss_blocks;
    int m_chunk;                                          // weight-gradient launch: 0 = one wave sums the whole minibatch of its tile (M <= 256); > 0: rows per
                                                          // blockIdx.y (multiple of 32): chunk c STORES its partial gradient into gslab + c * gslab_stride and one ordered
                                                          // pass adds the chunks (round 4: no atomics, two runs bitwise equal; no fused Adam)
    float* gslab; long long gslab_stride;                 // per-chunk gradient slabs of the large-minibatch form (engine workspace; nullptr when max_batch <= 256)
    // PPO2-style value clipping (mi_ppo_train_step_vclip; appended, so that no other field moves): the values recorded at collection time, indexed like returns
    // (nullptr: the plain value loss), and the range eps_v > 0 (+inf: never clips)
    const float* v_old; float clip_range_vf;
    // adaptive KL penalty (mi_ppo_train_step_kl; appended likewise).  kl_on: the penalised head / loss kernel runs (kl_coef >= 0; 0 measures only).  mean_old: the
    // old policy's action means per table row, indexed like logp_old (nullptr with logp_old == nullptr: formed in the step from net 2).  kl_partial: one float per
    // loss block, that block's sum of KL[m] (engine workspace).  mean_old_out: where the log pi_old pass of ppo_predict_head_kernel also stores its means
    // (mi_ppo_old_policy_cache; nullptr: nowhere)
    int kl_on; float kl_coef;
    int max_batch;                                        // the engine's, for the 2 GiB limit of the 32-bit byte offsets (host side only; in the padding behind kl_coef)
    const float* mean_old; float* kl_partial; float* mean_old_out;
    // behaviour cloning (mi_ppo_clone_step; appended likewise).  clone: 0 = a PPO step, 1 + kind = the clone head / loss kernel runs (1 "nll", 2 "mse") with
    // `actions` the expert's; returns == nullptr then means policy only.  n_wnets: the nets the backward half covers -- the layer-1 input-gradient grid and the
    // weight-gradient tiles in front of the spare wave: 2 in every step but the policy-only clone step, which runs net 0 alone (1)
    int clone, n_wnets;
    // demonstration term (mi_ppo_train_step_demo; appended likewise).  m_ppo: 0 = no demonstration rows; > 0: rows [0, m_ppo) of the M = m_ppo + M_demo rows of
    // the chain are PPO rows, the rest demonstration rows, and the ppo_head_demo kernels run.  The chain reads the staged rows (ppo_demo_stage_kernel: `states` of the
    // launches other than the head is the engine's [M, din] staging buffer, their row_idx is nullptr); the head kernel alone keeps row_idx / n_rows (the PPO tables)
    // and demo_row_idx / n_demo_rows (the demonstration tables demo_states / demo_actions; nullptr: contiguous).  demo_kind: 0 "nll", 1 "mse"; demo_coef = c_d;
    // inv_m_demo = 1 / M_demo(global).  demo_partial: two floats per loss block (the sums of l[m] and of the squared error over its demonstration rows);
    // demo_out: [demo_loss, c_d demo_loss, mean_sq_error] (mi_ppo_buffer(h, 4))
    int m_ppo, demo_kind, n_demo_rows; float demo_coef, inv_m_demo;
    // dual-clip PPO (mi_ppo_set_dual_clip), in the 4 bytes of padding behind inv_m_demo, so that no field moves: the constant c > 1 of the head / loss kernel's
    // surrogate, +inf with the setting off (fill_fused: never 0)
    float dual_clip;
    const float *demo_states, *demo_actions; const int* demo_row_idx; float *demo_partial, *demo_out;
};
static_assert(sizeof(PpoFusedParams) == 520, "PpoFusedParams: a field moved (the offsets of its fields are pinned by profiles/r28_ppo_wide_inputs.md)");
// (fields are appended only.  A kernel's arguments BEHIND the struct -- the predict and statistics heads -- move with its size, 456 -> 520 with the demonstration
// term; they are passed by value with every launch, so nothing else depends on where they sit: profiles/r36_demonstration_term.md)

}  // namespace mi

int mi_ppo_fused_partial_floats(int M);
int mi_ppo_fused_trunks(hipStream_t st, const mi::PpoFusedParams& q, bool x3);
bool mi_ppo_fused_shape_in_range(int A, int H2, int kin);
bool mi_ppo_fused_shape_in_wide_range(int A, int H2, int kin);      // the same limits on A and H2, kin <= 1024 (mi_ppo_set_wide_inputs)
int mi_ppo_fused_step(hipStream_t st, mi::PpoFusedParams& q, int fuse_adam, bool x3);      // x3: split-bf16 GEMM stages (MI_BF16X3)
int mi_ppo_fused_predict(hipStream_t st, mi::PpoFusedParams& q, const float* noise, int greedy, float* action, float* value);
int mi_ppo_fused_logp_old(hipStream_t st, mi::PpoFusedParams& q, float* out, bool x3);      // (q.mean_old_out set: the old policy's means as well)
int mi_ppo_fused_kl_stats(hipStream_t st, mi::PpoFusedParams& q, int accumulate, double* scratch, double* stats, bool x3);
// V(s) of M rows under the current theta, the value net alone; M may exceed q.max_batch (chunks).  q: fill_fused's block for the engine (states set, M ignored)
int mi_ppo_fused_values(hipStream_t st, const mi::PpoFusedParams& q, const int* row_idx, long long n_rows, long long M, float* values_out, bool x3);
// log pi_theta(a | s) of M rows under the current theta, the policy net alone; the same chunk loop and the same q
int mi_ppo_fused_logp(hipStream_t st, const mi::PpoFusedParams& q, const float* actions, const int* row_idx, long long n_rows, long long M, float* logp_out, bool x3);
int mi_ppo_fused_update_stats(hipStream_t st, mi::PpoFusedParams& q, int accumulate, double* scratch, double* stats, float* logp_new_out, float* value_out, bool x3);
// internal accessors of the two engines for the rollout step (rollout path only)
int mi_ppo_internal_fill(void* ppo_handle, mi::PpoFusedParams* q, const float* states, int M);
struct MiZeroList { float* p[3]; long long n[3]; };     // raw-sum buffers conv1's launch clears for the split-K layers behind it
int mi_rollout_conv(hipStream_t st, const float* x, const float* x_bias, int IH, int IW, int C, const float* w, int ldw, int N, int KH, int KW, float* out_raw, int flat_k);
int mi_rollout_conv1(hipStream_t st, const unsigned char* frame, const float* w, const float* bias, float* out, int IH, int IW, int Cs, int KH, int KW, int N, const MiZeroList* zero);
int mi_rollout_policy(hipStream_t st, const mi::PpoFusedParams& q, const float* mean_raw, const float* mean_bias, int z_dim, const float* measurements, const float* noise, int greedy, float* out);
// batched forms (n environments per launch; mi_rollout_step_batch)
int mi_rollout_conv1_batch(hipStream_t st, const unsigned char* frames, const float* w, const float* bias, float* out, int IH, int IW, int Cs, int KH, int KW, int N, int n, const MiZeroList* zero);
int mi_rollout_conv_batch(hipStream_t st, const float* x, const float* x_bias, int IH, int IW, int C, const float* w, int ldw, int N, int KH, int KW, float* out_raw, int flat_k, int n);
// One batched call -- any of the eleven mi_rollout_{step,value}_batch* / mi_mlp_rollout_{step,value}_batch* entries -- without its encoder chain, each field once.  The
// entry fills it and hands it to its engine's driver; the three functions below do everything that does not depend on the encoder.
struct MiRolloutCall {
    // name and form.  who: in front of every message; who_rec: in front of "null handle" and "missing tables" (another name for mi_rollout_step_batch_rec alone).
    // value_only: the value trunk and the value-only heads, out [n].  stacked: latent stacking.  must_record / must_normalise: the entry has no form without
    // table_rows / without obs_mean (the ConvVAE _rec, _norm and value entries); elsewhere a NULL there turns recording / normalising off
    const char *who, *who_rec; bool value_only, stacked, must_record, must_normalise;
    const float* measurements; int n_meas; const float* noise; int greedy, n; float* out;       // out [n][A + 1 + z_dim]
    // tables: call row e is also stored as row table_rows[e] of the horizon-batch tables (rows outside [0, n_table_rows) are skipped).  tab_states takes the state the
    // trunks read, tab_raw_states the raw one beside a normalised one; the value-only call writes tab_final_values alone
    const int* table_rows; long long n_table_rows; float *tab_states, *tab_raw_states, *tab_actions, *tab_values, *tab_final_values;
    // running observation normalisation: fp32 mean / inv_std [din] on the device, the clamp, and (not stacked) the caller's n x din buffer the normalised rows go to
    const float *obs_mean, *obs_inv_std; float obs_clip; float* nstate;
    // latent stacking: the state is [z_t | the latent_stack - 1 latents before it | measurements].  hist: fp32 [n_lanes][latent_stack - 1][z_dim] on the device, slot 0 =
    // the latent of the lane's previous step; lanes / first: int32 [n] (the step's input buffer); sstate: the caller's n x din buffer trunk layer 1 reads (the normalised
    // rows with obs_mean: the normaliser runs inside the stack kernel and nstate is unused); older: [n][(latent_stack - 1) z_dim] or NULL, where the older latents of
    // every row go (HBM or pinned host memory)
    int latent_stack; float* hist; int n_lanes; const int *lanes, *first; int advance; float *sstate, *older;
};
// the fields every entry has; the rest start as 0 / NULL
inline MiRolloutCall mi_rollout_call(const char* who, bool value_only, const float* measurements, int n_meas, const float* noise, int greedy, int n, float* out) {
    MiRolloutCall c = {};
    c.who = c.who_rec = who; c.value_only = value_only; c.measurements = measurements; c.n_meas = n_meas; c.noise = noise; c.greedy = greedy; c.n = n; c.out = out;
    return c;
}
inline void mi_rollout_call_stack(MiRolloutCall& c, int latent_stack, float* hist, int n_lanes, const int* lanes, const int* first, int advance, float* sstate, float* older) {
    c.stacked = true; c.latent_stack = latent_stack; c.hist = hist; c.n_lanes = n_lanes; c.lanes = lanes; c.first = first; c.advance = advance; c.sstate = sstate; c.older = older;
}
int mi_rollout_fail(int code, const char* who, const char* text);       // records "<who>: <text>" and returns code
// every refusal that reads neither handle (buffers, tables, normaliser, stack, the range of n), before any launch: MI_ERR_ARG with its message, or MI_OK
int mi_rollout_call_check(const MiRolloutCall& c, const void* frames, const void* scratch);
// the PPO side: fills q for c.n rows (refusing a policy whose input size, action count or max_batch does not fit the call) and entries 1 and 2 of the zero list -- the
// trunks' raw sums [net][n][H], or with value_only the value net's halves alone.  Entry 0 is the encoder's
int mi_rollout_call_prepare(const MiRolloutCall& c, void* ppo_h, const float* mean_raw, int z_dim, mi::PpoFusedParams* q, MiZeroList* zero);
// the launches behind the encoder: the normaliser or the stack kernel (trunk layer 1 then reads its rows), the two trunk stages (value_only: the value net at half the
// grid), and the plain, the recording or the value-only heads
int mi_rollout_call_finish(hipStream_t st, const MiRolloutCall& c, const mi::PpoFusedParams& q, const float* mean_raw, const float* mean_bias, int z_dim);
// layer 1 of the MlpVAE encoder from the camera bytes of n environments (rollout_mlp.hip; mi_mlp_rollout_step_batch): clears `zero` -- the raw-sum buffers of the whole
// call, raw1 among them -- in a launch of its own, then adds frames / 255 x w1 [S][N1] onto raw1 [n][N1] (fp32 atomics).  frames: 4-byte aligned.
int mi_rollout_mlp_layer1(hipStream_t st, const unsigned char* frames, const float* w1, float* raw1, int S, int N1, int n, const MiZeroList* zero);
