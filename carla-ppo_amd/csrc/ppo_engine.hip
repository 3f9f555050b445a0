// ppo_engine.hip — PPO policy/value network: predict and one minibatch-SGD step behind the C ABI.
// Mirrors PolicyGraph + PPO (reference ppo.py:16-66,112-147,218-251,275-276) with utils.build_mlp (utils.py:25-28):
//   pi: s -> dense 500 relu -> dense 300 relu -> action_mean (tanh, rescaled to [low,high]) ; free action_logstd
//   V : s -> dense 500 relu -> dense 300 relu -> value
// fp32 storage + exact-fp32 MFMA (the net is 369 505 parameters; the step is launch-latency bound, not MFMA bound).
// The state dimension is padded to a multiple of 8 on the device (zero rows in the first-layer kernels).
#include <stdlib.h>
#include "common.hpp"
#include "mi_internal.hpp"
#include "mi355_carla.h"
#include "ppo_fused.hpp"

using namespace mi;

namespace {

constexpr int PPO_TENSORS = 13;   // dense{k,b} dense_1{k,b} action_mean{k,b} action_logstd dense_2{k,b} dense_3{k,b} value{k,b}

inline long long pad8(long long n) { return (n + 7) / 8 * 8; }

struct PpoEngine {
    MiPpoDesc d;
    int kin;                                   // padded input dim
    long long off[PPO_TENSORS], size[PPO_TENSORS], total;
    float *params, *params_old, *grads, *m, *v;
    char* ws;
    // workspace offsets (bytes)
    long long s_pad, h1, h2, g1, g2, u, vraw, h1o, h2o, uo, du, dv, dh2, dh1, dg2, dg1, partial, losses, mean, low, high, ws_total;
    long long f_gslab;                            // per-chunk gradient slabs of the large-minibatch step (max_batch > 256): [ceil(max_batch / 256)][total]
    long long gn_part, clip;                      // global-norm clipping: the block partials of the sum of squares (doubles), and {norm, scale, c, 0} of the last norm (mi_ppo_buffer(h, 2))
    float max_grad_norm;                          // 0 (calloc: the default): no clipping; > 0 or +inf: mi_ppo_apply_adam clips by the global norm (mi_ppo_set_max_grad_norm)
    long long f_klpart;                           // KL penalty (mi_ppo_train_step_kl): one float per loss block
    long long f_demopart, f_demo;                 // demonstration term (mi_ppo_train_step_demo): two floats per loss block, and [demo_loss, c_d demo_loss, mean_sq_error] (mi_ppo_buffer(h, 4))
    long long wg_scr[2], wg_bytes;                // per-layer path: row-split slabs of its filter and bias gradients (mi_gemm_wgrad_bias_ws), one piece per stream of the backward pass
    long long f_h1, f_h2, f_dh1, f_dh2, f_part;   // fused step (ppo_fused.hip): [3][M][H1], [3][M][H2], [2][M][H1], [2][M][H2], loss-block partials
    int last_M;
    int precision;                                // MI_F32 (calloc: the default) or MI_BF16X3 (mi_ppo_set_precision): which instantiation of the fused GEMM stages runs
    float dual_clip;                              // 0 (calloc: the default): the plain surrogate; > 1 or +inf: dual-clip PPO in every fused step (mi_ppo_set_dual_clip)
    int wide;                                     // 0 (calloc: the default): the fused range ends at kin = 96; 1 / 2: at kin = 1024 (mi_ppo_set_wide_inputs).  Routing only
    hipStream_t side; hipEvent_t ev_fork, ev_join; int side_ok;     // second stream of the forked minibatch step (0 = not tried, 1 = ok, -1 = unavailable)
    float* P(int t) const { return params + off[t]; }
    float* PO(int t) const { return params_old + off[t]; }
    float* G(int t) const { return grads + off[t]; }
    void* at(long long o) const { return ws + o; }
};

void layout(PpoEngine& e) {
    const MiPpoDesc& d = e.d;
    e.kin = (d.input_dim + 7) / 8 * 8;
    long long o = 0; int t = 0;
    auto add = [&](long long n) { e.off[t] = o; e.size[t] = n; o += pad8(n); ++t; };
    add((long long)e.kin * d.h1); add(d.h1); add((long long)d.h1 * d.h2); add(d.h2); add((long long)d.h2 * d.num_actions); add(d.num_actions);
    add(d.num_actions);
    add((long long)e.kin * d.h1); add(d.h1); add((long long)d.h1 * d.h2); add(d.h2); add(d.h2); add(1);
    e.total = o;
    const long long M = d.max_batch;
    long long w = 0;
    auto wa = [&](long long bytes) { long long r = w; w += (bytes + 255) / 256 * 256; return r; };
    e.s_pad = wa(M * e.kin * 4);
    e.h1 = wa(M * d.h1 * 4); e.h2 = wa(M * d.h2 * 4); e.g1 = wa(M * d.h1 * 4); e.g2 = wa(M * d.h2 * 4);
    e.u = wa(M * d.num_actions * 4); e.vraw = wa(M * 4);
    e.h1o = wa(M * d.h1 * 4); e.h2o = wa(M * d.h2 * 4); e.uo = wa(M * d.num_actions * 4);
    e.du = wa(M * d.num_actions * 4); e.dv = wa(M * 4);
    e.dh2 = wa(M * d.h2 * 4); e.dh1 = wa(M * d.h1 * 4); e.dg2 = wa(M * d.h2 * 4); e.dg1 = wa(M * d.h1 * 4);
    e.partial = wa((long long)mi_ppo_loss_partial_floats((int)M) * 4);
    e.losses = wa(256); e.mean = wa(M * d.num_actions * 4); e.low = wa(256); e.high = wa(256);
    e.f_h1 = wa(3 * M * d.h1 * 4); e.f_h2 = wa(3 * M * d.h2 * 4); e.f_dh1 = wa(2 * M * d.h1 * 4); e.f_dh2 = wa(2 * M * d.h2 * 4);
    e.f_part = wa((long long)mi_ppo_fused_partial_floats((int)M) * 4);
    e.f_gslab = wa(M > 256 ? ((M + 255) / 256) * e.total * 4 : 0);
    e.gn_part = wa(MI_GRAD_NORM_BLOCKS * 8); e.clip = wa(16);
    e.f_klpart = wa(((M + 31) / 32) * 4);
    e.f_demopart = wa(((M + 31) / 32) * 8); e.f_demo = wa(16);
    // the per-layer path's filter gradients, with the bias gradient as one more row of the same product (mi_gemm_wgrad_bias_ws: no column-sum launches), sum their
    // row splits through slabs in a fixed order, not through fp32 atomics: two runs are bitwise equal, as on the fused path.  One piece per stream, sized for the
    // largest layer of a side at the row count with the most splits (the launches of a side are ordered on its stream)
    e.wg_bytes = 0;
    {
        const int kn[4][2] = {{d.h2, d.num_actions}, {d.h1, d.h2}, {e.kin, d.h1}, {d.h2, 1}};
        for (int i = 0; i < 4; ++i) { const long long nb = mi_gemm_wgrad_scratch_bytes(MI_F32, 1 << 20, kn[i][0], kn[i][1]); if (nb > e.wg_bytes) e.wg_bytes = nb; }
    }
    e.wg_scr[0] = wa(e.wg_bytes); e.wg_scr[1] = wa(e.wg_bytes);
    e.ws_total = w;
}

bool valid_desc(const MiPpoDesc* d) {
    return d && d->max_batch >= 1 && d->input_dim >= 1 && d->num_actions >= 1 && d->num_actions <= 8 && d->h1 % 4 == 0 && d->h2 % 4 == 0 && d->h1 > 0 && d->h2 > 0;
}

// states [M, input_dim] -> zero-padded [M, kin]
__global__ void pad_states_kernel(const float* __restrict__ s, int M, int din, int kin, float* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= M * kin) return;
    const int r = i / kin, c = i - r * kin;
    out[i] = c < din ? s[(long long)r * din + c] : 0.f;
}

// gradient through the two tiny heads back into the trunks (K = num_actions / 1 is below the MFMA vector width):
//   dh2[m,j] = (h2>0) * sum_a du[m,a] * Wm[j,a] ;  dg2[m,j] = (g2>0) * dv[m] * Wv[j]
__global__ void head_dgrad_kernel(const float* __restrict__ du, const float* __restrict__ dv, const float* __restrict__ Wm,
                                  const float* __restrict__ Wv, const float* __restrict__ h2, const float* __restrict__ g2,
                                  int M, int H, int A, float* __restrict__ dh2, float* __restrict__ dg2) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= M * H) return;
    const int m = i / H, j = i - m * H;
    float s = 0.f;
    for (int a = 0; a < A; ++a) s += du[(long long)m * A + a] * Wm[(long long)j * A + a];
    dh2[i] = h2[i] > 0.f ? s : 0.f;
    dg2[i] = g2[i] > 0.f ? dv[m] * Wv[j] : 0.f;
}

#define CK(call) do { int rc__ = (call); if (rc__ != MI_OK) return rc__; } while (0)

// the fused kernels serve the shapes they were built for (the reference's 500 / 300 trunk, <= 8 actions, and the input widths the engine's mode allows:
// mi_ppo_set_wide_inputs); anything else takes the per-layer path
bool fused_enabled(const PpoEngine* e);

bool fused_enabled(const PpoEngine* e) {
    if (!knob(K_PPO_FUSED)) return false;
    return e->wide ? mi_ppo_fused_shape_in_wide_range(e->d.num_actions, e->d.h2, e->kin) : mi_ppo_fused_shape_in_range(e->d.num_actions, e->d.h2, e->kin);
}

bool x3(const PpoEngine* e) { return e->precision == MI_BF16X3; }

bool clipping(const PpoEngine* e) { return e->max_grad_norm > 0.f; }

bool dual_clipping(const PpoEngine* e) { return e->dual_clip > 0.f; }

// the ordered sum of squares over the 13 variables of the gradient buffer (not the alignment gaps behind the odd-sized ones) -> MI_GRAD_NORM_BLOCKS partials
int grad_sumsq(PpoEngine* e, void* stream, int tensors = PPO_TENSORS) {
    return mi_grad_sumsq((hipStream_t)stream, e->grads, e->off, e->size, tensors, (double*)e->at(e->gn_part));
}

constexpr int PPO_POLICY_TENSORS = 7;                 // variables 0..6 (the policy net and action_logstd) lie in front of 7..12 (the value net) in the flat buffers

// tf.train.AdamOptimizer over the first `tensors` variables of the flat buffers: all 13 (mi_ppo_apply_adam), or the policy's prefix (the policy-only clone step:
// the value net's parameters and both of its slots are not touched, where a zero gradient would still decay the slots and move the parameters)
int adam_prefix(PpoEngine* e, void* stream, int tensors, float alpha, float beta1, float beta2, float epsilon) {
    const long long n = tensors == PPO_TENSORS ? e->total : e->off[tensors];
    if (clipping(e)) {      // two launches: the ordered sum of squares, then Adam on g * scale with the factor formed from the partials by every block
        CK(grad_sumsq(e, stream, tensors));
        return mi_adam_tf_flat_clipped((hipStream_t)stream, e->params, e->m, e->v, e->grads, n, alpha, beta1, beta2, epsilon,
                                       (const double*)e->at(e->gn_part), e->max_grad_norm, (float*)e->at(e->clip), 1);
    }
    return mi_adam_tf_flat(stream, e->params, e->m, e->v, e->grads, n, alpha, beta1, beta2, epsilon, nullptr, 1);
}

void fill_fused(const PpoEngine* e, PpoFusedParams& q, const float* states, int M) {
    const MiPpoDesc& d = e->d;
    q = PpoFusedParams{};
    q.theta = e->params; q.theta_old = e->params_old; q.adam_m = e->m; q.adam_v = e->v; q.grads = e->grads;
    for (int i = 0; i < 13; ++i) q.off[i] = e->off[i];
    q.kin = e->kin; q.din = d.input_dim; q.H1 = d.h1; q.H2 = d.h2; q.A = d.num_actions; q.M = M; q.n_params = e->total;
    q.states = states; q.low = (const float*)e->at(e->low); q.high = (const float*)e->at(e->high);
    q.h1 = (float*)e->at(e->f_h1); q.h2 = (float*)e->at(e->f_h2); q.dh1 = (float*)e->at(e->f_dh1); q.dh2 = (float*)e->at(e->f_dh2);
    q.du = (float*)e->at(e->du); q.dv = (float*)e->at(e->dv); q.partial = (float*)e->at(e->f_part); q.losses = (float*)e->at(e->losses);
    q.mean_out = (float*)e->at(e->mean); q.kl_partial = (float*)e->at(e->f_klpart);
    q.gslab = d.max_batch > 256 ? (float*)e->at(e->f_gslab) : nullptr; q.gslab_stride = e->total;      // (total is a multiple of 8 floats: pad8 per tensor)
    q.n_nets = 3; q.n_wnets = 2;
    q.clip_eps = d.clip_eps; q.value_scale = d.value_scale; q.entropy_scale = d.entropy_scale;      // (the live values: mi_ppo_set_loss_coefs writes e->d)
    q.dual_clip = dual_clipping(e) ? e->dual_clip : __builtin_inff();      // off: c = +inf, the branch of the head / loss kernel is never taken
    q.wide = e->wide; q.max_batch = d.max_batch;
}

// One minibatch step of the fused kernels, described ONCE for the six entries below (mi_ppo_forward_backward's fused branch, mi_ppo_train_step[_idx|_dp|_vclip|_kl]):
// what they put into PpoFusedParams behind fill_fused.  logp_old NULL: the step evaluates the old policy itself (three networks); row_idx given: states / actions /
// returns / advantage / logp_old (/ old_values / mean_old) are tables of n_rows rows gathered in-kernel; old_values given: the clipped value loss; kl: the KL penalty.
void fill_step(PpoEngine* e, PpoFusedParams& q, const float* states, const float* actions, const float* returns, const float* advantage, const float* logp_old,
               const int* row_idx, int n_rows, int M, float inv_m, float grad_scale, const float* old_values = nullptr, float clip_range_vf = 0.f,
               bool kl = false, float kl_coef = 0.f, const float* mean_old = nullptr) {
    fill_fused(e, q, states, M);
    q.actions = actions; q.returns = returns; q.adv = advantage; q.inv_m = inv_m; q.grad_scale = grad_scale;
    q.logp_old = logp_old; q.n_nets = logp_old ? 2 : 3;
    if (row_idx) { q.row_idx = row_idx; q.n_rows = n_rows; q.s_gath = (float*)e->at(e->s_pad); }
    if (old_values) { q.v_old = old_values; q.clip_range_vf = clip_range_vf; }
    if (kl) { q.kl_on = 1; q.kl_coef = kl_coef; q.mean_old = mean_old; }
    e->last_M = M;
}

// ... and the ONE route rule.  In-tile Adam (five launches, the optimiser update applied by the blocks that produce each gradient tile: no gradient buffer is written)
// iff the optimiser is wanted, there is no communicator, M <= 256 and clipping by the global norm is off.  Else the same five-kernel chain writes (not accumulates) the
// gradients into the flat buffer and the rest follows as launches of its own: clipping by the global norm needs the whole gradient at one moment, a communicator sums
// the buffer over the ranks, and large minibatches (the synthetic replay: 2048 rows per GPU) split the weight-gradient launch into row chunks of 256 whose partial sums
// are added in a fixed order (round 4: no atomics).  adam == 0 stops with the gradients in the buffer.
int route_step(PpoEngine* e, void* stream, PpoFusedParams& q, void* comm, int adam, float alpha, float beta1, float beta2, float epsilon) {
    if (adam && !comm && q.M <= 256 && !clipping(e)) {
        q.alpha = alpha; q.omb1 = 1.0f - beta1; q.omb2 = 1.0f - beta2; q.epsilon = epsilon;
        return mi_ppo_fused_step((hipStream_t)stream, q, 1, x3(e));
    }
    CK(mi_ppo_fused_step((hipStream_t)stream, q, 0, x3(e)));
    if (!adam) return MI_OK;
    // (the policy-only clone step: the all-reduce and the optimiser cover the policy's prefix of the flat buffers; the value net's range of the gradients is 0.0)
    const int tensors = q.n_wnets == 1 ? PPO_POLICY_TENSORS : PPO_TENSORS;
    if (comm) CK(mi_allreduce_sum_f32(comm, stream, e->grads, tensors == PPO_TENSORS ? e->total : e->off[tensors]));
    return adam_prefix(e, stream, tensors, alpha, beta1, beta2, epsilon);
}

int policy_fwd(PpoEngine* e, void* st, const float* prm, const long long* off, int M, void* h1, void* h2, void* u) {
    const MiPpoDesc& d = e->d;
    CK(mi_gemm_bias_act(st, MI_F32, e->at(e->s_pad), M, e->kin, prm + off[0], 0, d.h1, prm + off[1], 1, nullptr, h1, 1, 1));
    CK(mi_gemm_bias_act(st, MI_F32, h1, M, d.h1, prm + off[2], 0, d.h2, prm + off[3], 1, nullptr, h2, 1, 1));
    return mi_gemm_bias_act(st, MI_F32, h2, M, d.h2, prm + off[4], 0, d.num_actions, prm + off[5], 0, nullptr, u, 1, 1);
}
int value_fwd(PpoEngine* e, void* st, const float* prm, const long long* off, int M, void* vraw) {
    const MiPpoDesc& d = e->d;
    CK(mi_gemm_bias_act(st, MI_F32, e->at(e->s_pad), M, e->kin, prm + off[7], 0, d.h1, prm + off[8], 1, nullptr, e->at(e->g1), 1, 1));
    CK(mi_gemm_bias_act(st, MI_F32, e->at(e->g1), M, d.h1, prm + off[9], 0, d.h2, prm + off[10], 1, nullptr, e->at(e->g2), 1, 1));
    return mi_gemm_bias_act(st, MI_F32, e->at(e->g2), M, d.h2, prm + off[11], 0, 1, prm + off[12], 0, nullptr, vraw, 1, 1);
}
int trunk_fwd(PpoEngine* e, void* st, const float* prm, const long long* off, int M, bool value_branch, void* h1, void* h2, void* u, void* vraw) {
    CK(policy_fwd(e, st, prm, off, M, h1, h2, u));
    return value_branch ? value_fwd(e, st, prm, off, M, vraw) : MI_OK;
}

int stage_states(PpoEngine* e, void* st, const float* states, int M) {
    const int n = M * e->kin;
    hipLaunchKernelGGL(pad_states_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)st, states, M, e->d.input_dim, e->kin, (float*)e->at(e->s_pad));
    return mi_check_launch("pad_states");
}

}  // namespace

int mi_ppo_internal_fill(void* h, PpoFusedParams* q, const float* states, int M) {
    PpoEngine* e = (PpoEngine*)h;
    if (!e || M < 1 || M > e->d.max_batch) return mi_fail(MI_ERR_ARG, "ppo engine: bad handle or batch");
    fill_fused(e, *q, states, M);
    return MI_OK;
}

extern "C" {

int mi_ppo_desc_size(void) { return (int)sizeof(MiPpoDesc); }
int mi_ppo_tensor_count(void) { return PPO_TENSORS; }

long long mi_ppo_param_floats(const MiPpoDesc* d) {
    if (!valid_desc(d)) { mi_fail(MI_ERR_SHAPE, "mi_ppo_param_floats: bad descriptor (hidden sizes must be multiples of 4, 1..8 actions)"); return -1; }
    PpoEngine e; e.d = *d; layout(e); return e.total;
}

// device order: dense{kernel [kin,h1], bias} dense_1{k,b} action_mean{k,b} action_logstd dense_2{k,b} dense_3{k,b} value{k,b}
// (first-layer kernels carry kin - input_dim zero rows at the end)
int mi_ppo_param_layout(const MiPpoDesc* d, long long* offsets, long long* sizes, int n) {
    if (!valid_desc(d)) return mi_fail(MI_ERR_SHAPE, "mi_ppo_param_layout: bad descriptor");
    if (n != PPO_TENSORS) return mi_fail(MI_ERR_ARG, "mi_ppo_param_layout: expected 13 entries");
    PpoEngine e; e.d = *d; layout(e);
    for (int i = 0; i < PPO_TENSORS; ++i) { offsets[i] = e.off[i]; sizes[i] = e.size[i]; }
    return MI_OK;
}

long long mi_ppo_workspace_bytes(const MiPpoDesc* d) {
    if (!valid_desc(d)) { mi_fail(MI_ERR_SHAPE, "mi_ppo_workspace_bytes: bad descriptor"); return -1; }
    PpoEngine e; e.d = *d; layout(e); return e.ws_total;
}

void* mi_ppo_create(const MiPpoDesc* d, float* params, float* params_old, float* grads, float* adam_m, float* adam_v,
                    void* workspace, long long workspace_bytes, const float* action_low, const float* action_high) {
    if (!valid_desc(d)) { mi_fail(MI_ERR_SHAPE, "mi_ppo_create: bad descriptor"); return nullptr; }
    PpoEngine* e = (PpoEngine*)calloc(1, sizeof(PpoEngine));
    if (!e) { mi_fail(MI_ERR_STATE, "mi_ppo_create: out of host memory"); return nullptr; }
    e->d = *d; layout(*e);
    if (!params || !params_old || !workspace || workspace_bytes < e->ws_total || !action_low || !action_high) { free(e); mi_fail(MI_ERR_ARG, "mi_ppo_create: missing buffers or workspace too small"); return nullptr; }
    if ((((uintptr_t)params) | ((uintptr_t)params_old) | ((uintptr_t)workspace) | ((uintptr_t)grads)) & 255) { free(e); mi_fail(MI_ERR_ARG, "mi_ppo_create: buffers must be 256-byte aligned"); return nullptr; }
    e->params = params; e->params_old = params_old; e->grads = grads; e->m = adam_m; e->v = adam_v; e->ws = (char*)workspace;
    // action bounds are host arrays (gym Box.low/high); keep a device copy in the workspace
    if (hipMemcpy(e->at(e->low), action_low, d->num_actions * 4, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(e->at(e->high), action_high, d->num_actions * 4, hipMemcpyHostToDevice) != hipSuccess) {
        free(e); mi_fail(MI_ERR_STATE, "mi_ppo_create: copying action bounds failed"); return nullptr;
    }
    if (hipMemset(e->at(e->clip), 0, 16) != hipSuccess) { free(e); mi_fail(MI_ERR_STATE, "mi_ppo_create: clearing the clip record failed"); return nullptr; }
    return e;
}

void mi_ppo_destroy(void* h) {
    PpoEngine* e = (PpoEngine*)h;
    if (e && e->side_ok == 1) { hipStreamDestroy(e->side); hipEventDestroy(e->ev_fork); hipEventDestroy(e->ev_join); }
    free(h);
}

// 0 losses[5] (policy, value, entropy, total, mean ratio)   1 action_mean [M,A] of the last predict   2 {norm, scale, c, 0} of the last gradient norm
// 3 dv [M] of the last step: d loss / d value-head output per sample (workspace of the step; what value clipping zeroes)
// 4 [demo_loss, c_d demo_loss, mean_sq_error] of the last mi_ppo_train_step_demo
// 5 du [M, A] of the last step: d loss / d action-mean head output per sample (workspace of the step; what dual clip zeroes)
void* mi_ppo_buffer(void* h, int which) {
    PpoEngine* e = (PpoEngine*)h;
    if (!e) return nullptr;
    return which == 0 ? e->at(e->losses) : which == 1 ? e->at(e->mean) : which == 2 ? e->at(e->clip) : which == 3 ? e->at(e->dv) : which == 4 ? e->at(e->f_demo) : which == 5 ? e->at(e->du) : nullptr;
}

// PPO.update_old_policy (ppo.py:275-276): theta_old <- theta, one device copy of the flat buffer
int mi_ppo_update_old(void* h, void* stream) {
    PpoEngine* e = (PpoEngine*)h;
    if (!e) return mi_fail(MI_ERR_STATE, "ppo engine: null handle");
    if (hipMemcpyAsync(e->params_old, e->params, (size_t)e->total * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream) != hipSuccess)
        return mi_fail(MI_ERR_LAUNCH, "mi_ppo_update_old: copy failed");
    return MI_OK;
}

// PPO.predict (ppo.py:231-251): states [M,input_dim] -> action [M,A] (sampled+clipped, or greedy mean), value [M]
int mi_ppo_predict(void* h, void* stream, const float* states, int M, const float* noise, int greedy, float* action, float* value) {
    PpoEngine* e = (PpoEngine*)h;
    if (!e) return mi_fail(MI_ERR_STATE, "ppo engine: null handle");
    if (M < 1 || M > e->d.max_batch) return mi_fail(MI_ERR_ARG, "mi_ppo_predict: batch outside [1, max_batch]");
    if (!greedy && !noise) return mi_fail(MI_ERR_ARG, "mi_ppo_predict: sampling needs noise");
    if (fused_enabled(e)) {                                // 3 launches: layer 1, layer 2 (policy + value), heads
        PpoFusedParams q; fill_fused(e, q, states, M);
        return mi_ppo_fused_predict((hipStream_t)stream, q, noise, greedy, action, value);
    }
    CK(stage_states(e, stream, states, M));
    CK(trunk_fwd(e, stream, e->params, e->off, M, true, e->at(e->h1), e->at(e->h2), e->at(e->u), value));
    return mi_policy_head(stream, (const float*)e->at(e->u), e->P(6), noise, (const float*)e->at(e->low), (const float*)e->at(e->high),
                          M, e->d.num_actions, greedy, action, (float*)e->at(e->mean));
}

// Forward + loss + backward of one minibatch (the gradient half of PPO.train, ppo.py:218-229) into the flat gradient
// buffer (zero on entry).  inv_m = 1/M_global, grad_scale = M_local/M_global (data parallel; 1 for a single GPU).
int mi_ppo_forward_backward(void* h, void* stream, const float* states, const float* actions, const float* returns, const float* advantage,
                            int M, float inv_m, float grad_scale) {
    PpoEngine* e = (PpoEngine*)h;
    if (!e) return mi_fail(MI_ERR_STATE, "ppo engine: null handle");
    if (M < 1 || M > e->d.max_batch) return mi_fail(MI_ERR_ARG, "mi_ppo_forward_backward: batch outside [1, max_batch]");
    if (!e->grads) return mi_fail(MI_ERR_STATE, "mi_ppo_forward_backward: engine created without a gradient buffer");
    if (fused_enabled(e)) {                                // 5 launches; gradients written (not accumulated) into the flat buffer (M > 256: the row chunks' partial sums are added in a fixed order, round 4)
        PpoFusedParams q; fill_step(e, q, states, actions, returns, advantage, nullptr, nullptr, 0, M, inv_m, grad_scale);
        return route_step(e, stream, q, nullptr, 0, 0.f, 0.f, 0.f, 0.f);
    }
    if (x3(e)) return mi_fail(MI_ERR_SHAPE, "mi_ppo_forward_backward: the split-bf16 mode needs the fused kernels (no per-layer form of it)");
    if (dual_clipping(e)) return mi_fail(MI_ERR_SHAPE, "mi_ppo_forward_backward: dual clip is on (mi_ppo_set_dual_clip) and needs the fused kernels (no per-layer form of it)");
    const MiPpoDesc& d = e->d;
    void* st = stream;
    const int A = d.num_actions;
    // The step is ~28 launches of 5-9 us kernels that leave the chip almost empty, and the policy and value networks only meet in the loss:
    // the value side (and the old policy's forward) runs on a second stream.  Forward: policy(theta) | value(theta) + policy(theta_old);
    // backward: policy head + trunk | value head + trunk.  OFF by default (MI355_PPO_STREAMS=1 enables it): with device-resident minibatches
    // the step drops from 181 to 172 us, but the four event operations raise the host cost per step from 90 to 135 us, and the reference's
    // calling pattern (one host minibatch per train() call) is host-bound: 3.25 -> 3.6 ms per update of 16 steps.
    const int two_streams = knob(K_PPO_STREAMS);
    if (two_streams && !e->side_ok) {
        if (hipStreamCreateWithFlags(&e->side, hipStreamNonBlocking) == hipSuccess && hipEventCreateWithFlags(&e->ev_fork, hipEventDisableTiming) == hipSuccess &&
            hipEventCreateWithFlags(&e->ev_join, hipEventDisableTiming) == hipSuccess) e->side_ok = 1;
        else e->side_ok = -1;
    }
    const bool fork = two_streams && e->side_ok == 1;
    void* sw = fork ? (void*)e->side : st;
    auto release = [&]() { if (fork) { hipEventRecord(e->ev_fork, (hipStream_t)st); hipStreamWaitEvent(e->side, e->ev_fork, 0); } };
    auto join = [&]() { if (fork) { hipEventRecord(e->ev_join, e->side); hipStreamWaitEvent((hipStream_t)st, e->ev_join, 0); } };
    CK(stage_states(e, st, states, M));
    release();
    CK(policy_fwd(e, st, e->params, e->off, M, e->at(e->h1), e->at(e->h2), e->at(e->u)));
    CK(value_fwd(e, sw, e->params, e->off, M, e->at(e->vraw)));
    CK(policy_fwd(e, sw, e->params_old, e->off, M, e->at(e->h1o), e->at(e->h2o), e->at(e->uo)));
    join();
    CK(mi_ppo_loss_fwd_bwd(st, (const float*)e->at(e->u), (const float*)e->at(e->uo), e->P(6), e->PO(6), (const float*)e->at(e->vraw), actions, returns, advantage,
                           (const float*)e->at(e->low), (const float*)e->at(e->high), M, A, d.clip_eps, d.value_scale, d.entropy_scale, inv_m, grad_scale,
                           (float*)e->at(e->du), (float*)e->at(e->dv), (float*)e->at(e->partial), (float*)e->at(e->losses), e->G(6)));
    {   // gradient through the two heads into both trunks (needs du and dv: before the fork)
        const int n = M * d.h2;
        hipLaunchKernelGGL(head_dgrad_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)st, (const float*)e->at(e->du), (const float*)e->at(e->dv), e->P(4), e->P(11),
                           (const float*)e->at(e->h2), (const float*)e->at(e->g2), M, d.h2, A, (float*)e->at(e->dh2), (float*)e->at(e->dg2));
        CK(mi_check_launch("head_dgrad"));
    }
    release();
    // policy side (caller's stream): head, trunk.  (Filter + bias gradients: the ordered form, see layout())
    CK(mi_gemm_wgrad_bias_ws(st, MI_F32, e->at(e->h2), e->at(e->du), M, d.h2, A, e->G(4), e->G(5), e->at(e->wg_scr[0]), e->wg_bytes));
    CK(mi_gemm_wgrad_bias_ws(st, MI_F32, e->at(e->h1), e->at(e->dh2), M, d.h1, d.h2, e->G(2), e->G(3), e->at(e->wg_scr[0]), e->wg_bytes));
    CK(mi_gemm_bias_act(st, MI_F32, e->at(e->dh2), M, d.h2, e->P(2), 1, d.h1, nullptr, 0, e->at(e->h1), e->at(e->dh1), 1, 1));
    CK(mi_gemm_wgrad_bias_ws(st, MI_F32, e->at(e->s_pad), e->at(e->dh1), M, e->kin, d.h1, e->G(0), e->G(1), e->at(e->wg_scr[0]), e->wg_bytes));
    // value side (second stream): head, trunk
    CK(mi_gemm_wgrad_bias_ws(sw, MI_F32, e->at(e->g2), e->at(e->dv), M, d.h2, 1, e->G(11), e->G(12), e->at(e->wg_scr[1]), e->wg_bytes));
    CK(mi_gemm_wgrad_bias_ws(sw, MI_F32, e->at(e->g1), e->at(e->dg2), M, d.h1, d.h2, e->G(9), e->G(10), e->at(e->wg_scr[1]), e->wg_bytes));
    CK(mi_gemm_bias_act(sw, MI_F32, e->at(e->dg2), M, d.h2, e->P(9), 1, d.h1, nullptr, 0, e->at(e->g1), e->at(e->dg1), 1, 1));
    CK(mi_gemm_wgrad_bias_ws(sw, MI_F32, e->at(e->s_pad), e->at(e->dg1), M, e->kin, d.h1, e->G(7), e->G(8), e->at(e->wg_scr[1]), e->wg_bytes));
    join();
    e->last_M = M;
    return MI_OK;
}

// The whole of PPO.train's device work (ppo.py:218-229) in one call, single rank: forward of policy / value / old policy, losses, backward
// and tf.train.AdamOptimizer, as five launches (ppo_fused.hip); the optimiser update is applied by the blocks that produce each gradient
// tile, so no gradient buffer is involved.  logp_old != NULL: log pi_old(a|s) of these samples, computed once per horizon batch with
// mi_ppo_logp_old (theta_old is constant between two update_old_policy() calls): the old policy's forward pass is skipped.
int mi_ppo_train_step(void* h, void* stream, const float* states, const float* actions, const float* returns, const float* advantage, const float* logp_old,
                      int M, float inv_m, float grad_scale, float alpha, float beta1, float beta2, float epsilon) {
    PpoEngine* e = (PpoEngine*)h;
    if (!e) return mi_fail(MI_ERR_STATE, "ppo engine: null handle");
    if (M < 1 || M > e->d.max_batch) return mi_fail(MI_ERR_ARG, "mi_ppo_train_step: batch outside [1, max_batch]");
    if (!e->grads || !e->m || !e->v) return mi_fail(MI_ERR_STATE, "mi_ppo_train_step: engine created without optimiser buffers");
    if (!fused_enabled(e)) {                               // the per-layer pass (logp_old is not used), then Adam
        CK(mi_ppo_forward_backward(h, stream, states, actions, returns, advantage, M, inv_m, grad_scale));
        return mi_ppo_apply_adam(h, stream, alpha, beta1, beta2, epsilon);
    }
    PpoFusedParams q; fill_step(e, q, states, actions, returns, advantage, logp_old, nullptr, 0, M, inv_m, grad_scale);
    return route_step(e, stream, q, nullptr, 1, alpha, beta1, beta2, epsilon);
}

// 1: this engine's shape (num_actions, hidden sizes, input width) is inside the range of the fused kernels (csrc/ppo_fused.hip) and they are switched on, i.e.
// mi_ppo_train_step_idx / mi_ppo_logp_old will run; 0: only the per-layer path (mi_ppo_train_step / mi_ppo_forward_backward fall back to it by themselves;
// the _idx form has no per-layer equivalent: gather on the host side).  The host mirror asks before it picks the in-kernel gather.
int mi_ppo_fused_shape_ok(void* h) {
    PpoEngine* e = (PpoEngine*)h;
    return (e && fused_enabled(e)) ? 1 : 0;
}

// mi_ppo_train_step with the minibatch GATHER fused in: states / actions / returns / advantage / logp_old are the horizon-batch tables (n_rows rows;
// device resident for the whole update, train.py:175-207) and row_idx [M] (int32, device) names the rows of this minibatch -- the reference's
// `states[mb_idx]` fancy-indexing (train.py:199-204) happens inside the kernels that read the operands instead of as five gather launches per step.
int mi_ppo_train_step_idx(void* h, void* stream, const float* states, const float* actions, const float* returns, const float* advantage, const float* logp_old,
                          const int* row_idx, int n_rows, int M, float inv_m, float grad_scale, float alpha, float beta1, float beta2, float epsilon) {
    PpoEngine* e = (PpoEngine*)h;
    if (!e) return mi_fail(MI_ERR_STATE, "ppo engine: null handle");
    if (M < 1 || M > e->d.max_batch || n_rows < 1) return mi_fail(MI_ERR_ARG, "mi_ppo_train_step_idx: batch outside [1, max_batch] or empty tables");
    if (!row_idx) return mi_fail(MI_ERR_ARG, "mi_ppo_train_step_idx: missing row index (use mi_ppo_train_step for contiguous minibatches)");
    if (!e->grads || !e->m || !e->v) return mi_fail(MI_ERR_STATE, "mi_ppo_train_step_idx: engine created without optimiser buffers");
    if (!fused_enabled(e)) return mi_fail(MI_ERR_SHAPE, "mi_ppo_train_step_idx: needs the fused kernels (shape outside their range or MI355_PPO_FUSED=0): gather on the host side and call mi_ppo_train_step");
    PpoFusedParams q; fill_step(e, q, states, actions, returns, advantage, logp_old, row_idx, n_rows, M, inv_m, grad_scale);
    return route_step(e, stream, q, nullptr, 1, alpha, beta1, beta2, epsilon);
}

// One DATA-PARALLEL SGD step of PPO.train (ppo.py:218-229 behind train.py:193-207) in ONE call (round 6): the fused five-launch chain of
// mi_ppo_train_step[_idx] with the gradients left in the flat buffer (sums over this rank's M rows / M_global: inv_m = 1 / M_global, grad_scale = M / M_global), ONE
// all-reduce of that buffer (1.48 MB: one bucket, in stream order -- nothing of this step is left to overlap it with), tf.train.AdamOptimizer.  row_idx != NULL: the
// minibatch gather of train.py:199-204 stays inside the kernels (states / actions / returns / advantage / logp_old are this rank's horizon-batch tables of n_rows rows);
// row_idx == NULL: contiguous minibatch tensors (n_rows ignored).  comm: mi_comm_init (or a recording communicator).  Before round 6 the host issued
// forward_backward -> a blocking Python-side all-reduce -> apply_adam and gathered the rows itself whenever world_size > 1.
int mi_ppo_train_step_dp(void* h, void* comm, void* stream, const float* states, const float* actions, const float* returns, const float* advantage, const float* logp_old,
                         const int* row_idx, int n_rows, int M, float inv_m, float grad_scale, float alpha, float beta1, float beta2, float epsilon) {
    PpoEngine* e = (PpoEngine*)h;
    if (!e) return mi_fail(MI_ERR_STATE, "ppo engine: null handle");
    if (!comm) return mi_fail(MI_ERR_ARG, "mi_ppo_train_step_dp: null communicator (single rank: mi_ppo_train_step)");
    if (M < 1 || M > e->d.max_batch || (row_idx && n_rows < 1)) return mi_fail(MI_ERR_ARG, "mi_ppo_train_step_dp: batch outside [1, max_batch] or empty tables");
    if (!e->grads || !e->m || !e->v) return mi_fail(MI_ERR_STATE, "mi_ppo_train_step_dp: engine created without optimiser buffers");
    if (fused_enabled(e)) {                                // a communicator: the flat route at every M
        PpoFusedParams q; fill_step(e, q, states, actions, returns, advantage, logp_old, row_idx, n_rows, M, inv_m, grad_scale);
        return route_step(e, stream, q, comm, 1, alpha, beta1, beta2, epsilon);
    }
    if (row_idx) return mi_fail(MI_ERR_SHAPE, "mi_ppo_train_step_dp: the in-kernel gather needs the fused kernels (shape outside their range or MI355_PPO_FUSED=0): gather on the host side and pass row_idx = NULL");
    CK(mi_ppo_forward_backward(h, stream, states, actions, returns, advantage, M, inv_m, grad_scale));      // the per-layer pass (logp_old is not used)
    CK(mi_allreduce_sum_f32(comm, stream, e->grads, e->total));
    return mi_ppo_apply_adam(h, stream, alpha, beta1, beta2, epsilon);
}

// The minibatch step with the clipped value loss of PPO2 (include/mi355_carla.h; the definition is in ppo_fused.hip's head / loss kernel): ONE entry for the three
// existing forms -- row_idx == NULL: contiguous minibatch tensors as mi_ppo_train_step, row_idx != NULL: the tables (old_values among them) gathered in-kernel as
// mi_ppo_train_step_idx, comm != NULL: the all-reduce of the flat buffer in front of Adam as mi_ppo_train_step_dp -- and for mi_ppo_forward_backward's role
// (adam == 0: the gradients stay in the flat buffer).  adam == 1 takes the routes those entries take: the in-tile Adam for M <= 256 with clipping by the global norm
// off and no communicator, else the flat buffer and mi_ppo_apply_adam.  Fused kernels only: there is no per-layer form.
int mi_ppo_train_step_vclip(void* h, void* comm, void* stream, const float* states, const float* actions, const float* returns, const float* advantage,
                            const float* logp_old, const float* old_values, float clip_range_vf, const int* row_idx, int n_rows, int M,
                            float inv_m, float grad_scale, int adam, float alpha, float beta1, float beta2, float epsilon) {
    PpoEngine* e = (PpoEngine*)h;
    if (!e) return mi_fail(MI_ERR_STATE, "mi_ppo_train_step_vclip: null handle");
    // (what needs no engine is checked before the handle is looked at)
    if (M < 1 || (row_idx && n_rows < 1)) return mi_fail(MI_ERR_ARG, "mi_ppo_train_step_vclip: batch outside [1, max_batch] or empty tables");
    if (!old_values) return mi_fail(MI_ERR_ARG, "mi_ppo_train_step_vclip: missing old_values (an unclipped step: mi_ppo_train_step / _idx / _dp)");
    if (!(clip_range_vf > 0.f)) return mi_fail(MI_ERR_ARG, "mi_ppo_train_step_vclip: clip_range_vf is a positive float or +inf");
    if (adam != 0 && adam != 1) return mi_fail(MI_ERR_ARG, "mi_ppo_train_step_vclip: adam is 0 (stop with the gradients in the flat buffer) or 1 (apply the optimiser)");
    if (M > e->d.max_batch) return mi_fail(MI_ERR_ARG, "mi_ppo_train_step_vclip: batch outside [1, max_batch] or empty tables");
    if (!e->grads || (adam && (!e->m || !e->v))) return mi_fail(MI_ERR_STATE, "mi_ppo_train_step_vclip: engine created without gradient / optimiser buffers");
    if (!fused_enabled(e)) return mi_fail(MI_ERR_SHAPE, "mi_ppo_train_step_vclip: needs the fused kernels (shape outside their range or MI355_PPO_FUSED=0): there is no per-layer form of the clipped value loss");
    PpoFusedParams q; fill_step(e, q, states, actions, returns, advantage, logp_old, row_idx, n_rows, M, inv_m, grad_scale, old_values, clip_range_vf);
    return route_step(e, stream, q, comm, adam, alpha, beta1, beta2, epsilon);
}

// The minibatch step with the adaptive-KL penalty of the PPO paper added to the clipped surrogate (include/mi355_carla.h; the definition is in ppo_fused.hip's head /
// loss kernel): ONE entry for every form, as mi_ppo_train_step_vclip is -- row_idx NULL or not, comm NULL or not, adam 0 / 1, old_values NULL (the plain value loss)
// or the clipped one -- on the routes of that entry.  kl_coef = 0 measures: the KL slots are filled and nothing is added.  Fused kernels only.
int mi_ppo_train_step_kl(void* h, void* comm, void* stream, const float* states, const float* actions, const float* returns, const float* advantage,
                         const float* logp_old, const float* mean_old, float kl_coef, const float* old_values, float clip_range_vf,
                         const int* row_idx, int n_rows, int M, float inv_m, float grad_scale, int adam, float alpha, float beta1, float beta2, float epsilon) {
    PpoEngine* e = (PpoEngine*)h;
    if (!e) return mi_fail(MI_ERR_STATE, "mi_ppo_train_step_kl: null handle");
    // (what needs no engine is checked before the handle is looked at)
    if (M < 1 || (row_idx && n_rows < 1)) return mi_fail(MI_ERR_ARG, "mi_ppo_train_step_kl: batch outside [1, max_batch] or empty tables");
    if ((logp_old != nullptr) != (mean_old != nullptr))
        return mi_fail(MI_ERR_ARG, "mi_ppo_train_step_kl: logp_old and mean_old come together (mi_ppo_old_policy_cache) or are both NULL (the step evaluates the old policy)");
    if (!(kl_coef >= 0.f) || !(kl_coef <= 3.402823466e+38f)) return mi_fail(MI_ERR_ARG, "mi_ppo_train_step_kl: kl_coef is a finite float >= 0 (0: measure the KL, add nothing)");
    if (old_values && !(clip_range_vf > 0.f)) return mi_fail(MI_ERR_ARG, "mi_ppo_train_step_kl: with old_values, clip_range_vf is a positive float or +inf");
    if (adam != 0 && adam != 1) return mi_fail(MI_ERR_ARG, "mi_ppo_train_step_kl: adam is 0 (stop with the gradients in the flat buffer) or 1 (apply the optimiser)");
    if (M > e->d.max_batch) return mi_fail(MI_ERR_ARG, "mi_ppo_train_step_kl: batch outside [1, max_batch] or empty tables");
    if (!e->grads || (adam && (!e->m || !e->v))) return mi_fail(MI_ERR_STATE, "mi_ppo_train_step_kl: engine created without gradient / optimiser buffers");
    if (!fused_enabled(e)) return mi_fail(MI_ERR_SHAPE, "mi_ppo_train_step_kl: needs the fused kernels (shape outside their range or MI355_PPO_FUSED=0): there is no per-layer form of the KL penalty");
    PpoFusedParams q; fill_step(e, q, states, actions, returns, advantage, logp_old, row_idx, n_rows, M, inv_m, grad_scale, old_values, clip_range_vf, true, kl_coef, mean_old);
    return route_step(e, stream, q, comm, adam, alpha, beta1, beta2, epsilon);
}

// Behaviour cloning (include/mi355_carla.h; the definition is in ppo_fused.hip's clone head / loss kernel): ONE entry for every form, as mi_ppo_train_step_kl is --
// row_idx NULL or not, comm NULL or not, adam 0 / 1, returns NULL (policy only: the value net is neither run nor touched) or given (the value net is fitted to them)
// -- on route_step's routes.  Fused kernels only.
int mi_ppo_clone_step(void* h, void* comm, void* stream, const float* states, const float* expert_actions, const float* returns, int kind,
                      const int* row_idx, int n_rows, int M, float inv_m, float grad_scale, int adam, float alpha, float beta1, float beta2, float epsilon) {
    PpoEngine* e = (PpoEngine*)h;
    if (!e) return mi_fail(MI_ERR_STATE, "mi_ppo_clone_step: null handle");
    // (what needs no engine is checked before the handle is looked at)
    if (M < 1 || (row_idx && n_rows < 1)) return mi_fail(MI_ERR_ARG, "mi_ppo_clone_step: batch outside [1, max_batch] or empty tables");
    if (!states || !expert_actions) return mi_fail(MI_ERR_ARG, "mi_ppo_clone_step: missing buffers (states, expert_actions)");
    if (kind != 0 && kind != 1) return mi_fail(MI_ERR_ARG, "mi_ppo_clone_step: kind is 0 (the Gaussian negative log-likelihood) or 1 (the squared error of the mean)");
    if (adam != 0 && adam != 1) return mi_fail(MI_ERR_ARG, "mi_ppo_clone_step: adam is 0 (stop with the gradients in the flat buffer) or 1 (apply the optimiser)");
    if (M > e->d.max_batch) return mi_fail(MI_ERR_ARG, "mi_ppo_clone_step: batch outside [1, max_batch] or empty tables");
    if (!e->grads || (adam && (!e->m || !e->v))) return mi_fail(MI_ERR_STATE, "mi_ppo_clone_step: engine created without gradient / optimiser buffers");
    if (!fused_enabled(e)) return mi_fail(MI_ERR_SHAPE, "mi_ppo_clone_step: needs the fused kernels (shape outside their range or MI355_PPO_FUSED=0): there is no per-layer form of the clone step");
    PpoFusedParams q; fill_step(e, q, states, expert_actions, returns, nullptr, nullptr, row_idx, n_rows, M, inv_m, grad_scale);
    // no old policy (net 2 is not run), no advantage, no entropy term; policy only: net 0 alone through the whole chain
    q.clone = 1 + kind; q.entropy_scale = 0.f;
    q.n_nets = q.n_wnets = returns ? 2 : 1;
    return route_step(e, stream, q, comm, adam, alpha, beta1, beta2, epsilon);
}

// The PPO step with a demonstration term (include/mi355_carla.h; the definition is in ppo_fused.hip's head / loss kernel, DEMO): M PPO rows and M_demo demonstration
// rows in ONE fused chain over M + M_demo rows -- a staging launch gathers the state rows of the two tables, the trunks, ppo_head_demo*_kernel (per sample the PPO or the
// clone arithmetic), the layer-1 input gradient, the weight gradients -- one gradient, one Adam update.  ONE entry for every form, as mi_ppo_train_step_kl is, on
// route_step's routes with M + M_demo in the place of M.  Every refusal stands in front of the first launch.  Fused kernels only.
int mi_ppo_train_step_demo(void* h, void* comm, void* stream, const float* states, const float* actions, const float* returns, const float* advantage,
                           const float* logp_old, const float* mean_old, int kl_on, float kl_coef, const float* old_values, float clip_range_vf,
                           const int* row_idx, int n_rows, int M, const float* demo_states, const float* demo_actions, const int* demo_row_idx, int n_demo_rows, int M_demo,
                           int demo_kind, float demo_coef, float inv_m_demo, float inv_m, float grad_scale, int adam, float alpha, float beta1, float beta2, float epsilon) {
    PpoEngine* e = (PpoEngine*)h;
    if (!e) return mi_fail(MI_ERR_STATE, "mi_ppo_train_step_demo: null handle");
    // (what needs no engine is checked before the handle is looked at)
    if (M < 1 || (row_idx && n_rows < 1)) return mi_fail(MI_ERR_ARG, "mi_ppo_train_step_demo: batch outside [1, max_batch] or empty tables");
    if (M_demo < 1 || (demo_row_idx && n_demo_rows < 1)) return mi_fail(MI_ERR_ARG, "mi_ppo_train_step_demo: M_demo is at least 1 and the demonstration tables are not empty");
    if (!states || !actions || !returns || !advantage) return mi_fail(MI_ERR_ARG, "mi_ppo_train_step_demo: missing buffers (states, actions, returns, advantage)");
    if (!demo_states || !demo_actions) return mi_fail(MI_ERR_ARG, "mi_ppo_train_step_demo: missing buffers (demo_states, demo_actions)");
    if (demo_kind != 0 && demo_kind != 1) return mi_fail(MI_ERR_ARG, "mi_ppo_train_step_demo: demo_kind is 0 (the Gaussian negative log-likelihood) or 1 (the squared error of the mean)");
    if (!(demo_coef >= 0.f) || !(demo_coef <= 3.402823466e+38f)) return mi_fail(MI_ERR_ARG, "mi_ppo_train_step_demo: demo_coef is a finite float >= 0");
    if (!(inv_m_demo > 0.f)) return mi_fail(MI_ERR_ARG, "mi_ppo_train_step_demo: inv_m_demo is 1 / M_demo(global), a positive float");
    if (kl_on != 0 && kl_on != 1) return mi_fail(MI_ERR_ARG, "mi_ppo_train_step_demo: kl_on is 0 (no KL penalty) or 1");
    if (kl_on && (logp_old != nullptr) != (mean_old != nullptr))
        return mi_fail(MI_ERR_ARG, "mi_ppo_train_step_demo: with kl_on, logp_old and mean_old come together (mi_ppo_old_policy_cache) or are both NULL (the step evaluates the old policy)");
    if (kl_on && (!(kl_coef >= 0.f) || !(kl_coef <= 3.402823466e+38f))) return mi_fail(MI_ERR_ARG, "mi_ppo_train_step_demo: kl_coef is a finite float >= 0 (0: measure the KL, add nothing)");
    if (old_values && !(clip_range_vf > 0.f)) return mi_fail(MI_ERR_ARG, "mi_ppo_train_step_demo: with old_values, clip_range_vf is a positive float or +inf");
    if (adam != 0 && adam != 1) return mi_fail(MI_ERR_ARG, "mi_ppo_train_step_demo: adam is 0 (stop with the gradients in the flat buffer) or 1 (apply the optimiser)");
    if ((long long)M + M_demo > e->d.max_batch) return mi_fail(MI_ERR_ARG, "mi_ppo_train_step_demo: M + M_demo exceeds max_batch");
    if (!e->grads || (adam && (!e->m || !e->v))) return mi_fail(MI_ERR_STATE, "mi_ppo_train_step_demo: engine created without gradient / optimiser buffers");
    if (!fused_enabled(e)) return mi_fail(MI_ERR_SHAPE, "mi_ppo_train_step_demo: needs the fused kernels (shape outside their range or MI355_PPO_FUSED=0): there is no per-layer form of the demonstration term");
    PpoFusedParams q; fill_step(e, q, states, actions, returns, advantage, logp_old, row_idx, n_rows, M + M_demo, inv_m, grad_scale, old_values, clip_range_vf,
                                kl_on != 0, kl_coef, kl_on ? mean_old : nullptr);
    q.m_ppo = M; q.demo_kind = demo_kind; q.demo_coef = demo_coef; q.inv_m_demo = inv_m_demo;
    q.demo_states = demo_states; q.demo_actions = demo_actions; q.demo_row_idx = demo_row_idx; q.n_demo_rows = n_demo_rows;
    q.demo_partial = (float*)e->at(e->f_demopart); q.demo_out = (float*)e->at(e->f_demo);
    q.s_gath = (float*)e->at(e->s_pad);                    // the staged rows of both tables (with and without row lists)
    return route_step(e, stream, q, comm, adam, alpha, beta1, beta2, epsilon);
}

// mi_ppo_logp_old that keeps the old policy's action means as well: logp_out [M] (bit for bit mi_ppo_logp_old's), mean_out [M, A] -- the two tables of the KL penalty
int mi_ppo_old_policy_cache(void* h, void* stream, const float* states, const float* actions, int M, float* logp_out, float* mean_out) {
    PpoEngine* e = (PpoEngine*)h;
    if (!e) return mi_fail(MI_ERR_STATE, "mi_ppo_old_policy_cache: null handle");
    if (M < 1 || M > e->d.max_batch) return mi_fail(MI_ERR_ARG, "mi_ppo_old_policy_cache: batch outside [1, max_batch]");
    if (!states || !actions || !logp_out || !mean_out) return mi_fail(MI_ERR_ARG, "mi_ppo_old_policy_cache: missing buffers");
    if (!fused_enabled(e)) return mi_fail(MI_ERR_SHAPE, "mi_ppo_old_policy_cache: needs the fused kernels (shape outside their range or MI355_PPO_FUSED=0)");
    PpoFusedParams q; fill_fused(e, q, states, M);
    q.actions = actions; q.mean_old_out = mean_out;
    return mi_ppo_fused_logp_old((hipStream_t)stream, q, logp_out, x3(e));
}

// The exact-KL statistics pass (include/mi355_carla.h): the sums behind the mean / spread of the closed-form KL(pi_old || pi_theta) of M gathered table rows under
// the CURRENT theta against the cached old means -- forward only, ordered reduction, nothing of the training state is written.
long long mi_ppo_kl_stats_scratch_doubles(int M) { return (long long)MI_PPO_N_KL_STATS * (M < 1 ? 1 : (M + 31) / 32); }

int mi_ppo_kl_stats_idx(void* h, void* stream, const float* states, const float* mean_old, const int* row_idx, int n_rows, int M, int accumulate, double* scratch, double* stats) {
    PpoEngine* e = (PpoEngine*)h;
    if (!e) return mi_fail(MI_ERR_STATE, "mi_ppo_kl_stats_idx: null handle");
    // (what needs no engine is checked before the handle is looked at)
    if (M < 1 || n_rows < 1) return mi_fail(MI_ERR_ARG, "mi_ppo_kl_stats_idx: batch outside [1, max_batch] or empty tables");
    if (!states || !mean_old || !row_idx || !scratch || !stats) return mi_fail(MI_ERR_ARG, "mi_ppo_kl_stats_idx: missing buffers (states, mean_old, row_idx, scratch, stats)");
    if (accumulate != 0 && accumulate != 1) return mi_fail(MI_ERR_ARG, "mi_ppo_kl_stats_idx: accumulate is 0 (store the sums) or 1 (add them to stats)");
    if (M > e->d.max_batch) return mi_fail(MI_ERR_ARG, "mi_ppo_kl_stats_idx: batch outside [1, max_batch] or empty tables");
    if (!fused_enabled(e)) return mi_fail(MI_ERR_SHAPE, "mi_ppo_kl_stats_idx: needs the fused kernels (shape outside their range or MI355_PPO_FUSED=0)");
    PpoFusedParams q; fill_fused(e, q, states, M);
    q.mean_old = mean_old; q.row_idx = row_idx; q.n_rows = n_rows;
    return mi_ppo_fused_kl_stats((hipStream_t)stream, q, accumulate, scratch, stats, x3(e));
}

// log pi_old(a | s) of M samples under theta_old -> out [M] (the per-horizon cache for mi_ppo_train_step)
int mi_ppo_logp_old(void* h, void* stream, const float* states, const float* actions, int M, float* out) {
    PpoEngine* e = (PpoEngine*)h;
    if (!e) return mi_fail(MI_ERR_STATE, "ppo engine: null handle");
    if (M < 1 || M > e->d.max_batch) return mi_fail(MI_ERR_ARG, "mi_ppo_logp_old: batch outside [1, max_batch]");
    PpoFusedParams q; fill_fused(e, q, states, M);
    q.actions = actions;
    return mi_ppo_fused_logp_old((hipStream_t)stream, q, out, x3(e));
}

// Per-epoch update diagnostics (include/mi355_carla.h): the sums behind approx KL (k3 and k1), clipped fraction, mean ratio, value error and explained variance of M
// gathered table rows under the CURRENT theta against the cached log pi_old -- forward only, ordered reduction, nothing of the training state is written.
long long mi_ppo_update_stats_scratch_doubles(int M) { return (long long)MI_PPO_N_STATS * (M < 1 ? 1 : (M + 31) / 32); }

int mi_ppo_update_stats_idx(void* h, void* stream, const float* states, const float* actions, const float* returns, const float* logp_old,
                            const int* row_idx, int n_rows, int M, int accumulate, double* scratch, double* stats, float* logp_new_out, float* value_out) {
    PpoEngine* e = (PpoEngine*)h;
    if (!e) return mi_fail(MI_ERR_STATE, "mi_ppo_update_stats_idx: null handle");
    // (what needs no engine is checked before the handle is looked at)
    if (M < 1 || n_rows < 1) return mi_fail(MI_ERR_ARG, "mi_ppo_update_stats_idx: batch outside [1, max_batch] or empty tables");
    {
        const void* need[7] = {states, actions, returns, logp_old, row_idx, scratch, stats};
        static const char* const msg[7] = {"mi_ppo_update_stats_idx: missing buffers (states)", "mi_ppo_update_stats_idx: missing buffers (actions)",
                                           "mi_ppo_update_stats_idx: missing buffers (returns)", "mi_ppo_update_stats_idx: missing buffers (logp_old)",
                                           "mi_ppo_update_stats_idx: missing buffers (row_idx)", "mi_ppo_update_stats_idx: missing buffers (scratch)",
                                           "mi_ppo_update_stats_idx: missing buffers (stats)"};
        for (int i = 0; i < 7; ++i) if (!need[i]) return mi_fail(MI_ERR_ARG, msg[i]);
    }
    if (accumulate != 0 && accumulate != 1) return mi_fail(MI_ERR_ARG, "mi_ppo_update_stats_idx: accumulate is 0 (store the sums) or 1 (add them to stats)");
    if (M > e->d.max_batch) return mi_fail(MI_ERR_ARG, "mi_ppo_update_stats_idx: batch outside [1, max_batch] or empty tables");
    if (!fused_enabled(e)) return mi_fail(MI_ERR_SHAPE, "mi_ppo_update_stats_idx: needs the fused kernels (shape outside their range or MI355_PPO_FUSED=0)");
    PpoFusedParams q; fill_fused(e, q, states, M);
    q.actions = actions; q.returns = returns; q.logp_old = logp_old;
    q.row_idx = row_idx; q.n_rows = n_rows;
    return mi_ppo_fused_update_stats((hipStream_t)stream, q, accumulate, scratch, stats, logp_new_out, value_out, x3(e));
}

// V(s) of table rows under the CURRENT theta (include/mi355_carla.h): the value net alone, forward only -- what the rollout buffers refresh their value table with
// before every later epoch of an update.  M may exceed max_batch (the chunk loop is mi_ppo_fused_values').  Nothing of the training state is written.
int mi_ppo_values_idx(void* h, void* stream, const float* states, const int* row_idx, long long n_rows, long long M, float* values_out) {
    // (what needs no engine is checked before the handle is looked at)
    if (M < 1 || n_rows < 1) return mi_fail(MI_ERR_ARG, "mi_ppo_values_idx: no rows (M < 1) or an empty table (n_rows < 1)");
    if (!states) return mi_fail(MI_ERR_ARG, "mi_ppo_values_idx: missing buffers (states)");
    if (!values_out) return mi_fail(MI_ERR_ARG, "mi_ppo_values_idx: missing buffers (values_out)");
    if (!row_idx && M > n_rows) return mi_fail(MI_ERR_ARG, "mi_ppo_values_idx: without a row list the rows are 0 .. M - 1 of the table: M exceeds n_rows");
    PpoEngine* e = (PpoEngine*)h;
    if (!e) return mi_fail(MI_ERR_STATE, "mi_ppo_values_idx: null handle");
    if (!fused_enabled(e)) return mi_fail(MI_ERR_SHAPE, "mi_ppo_values_idx: needs the fused kernels (shape outside their range or MI355_PPO_FUSED=0)");
    PpoFusedParams q; fill_fused(e, q, states, 1);
    return mi_ppo_fused_values((hipStream_t)stream, q, row_idx, n_rows, M, values_out, x3(e));
}

// log pi_theta(a | s) of table rows under the CURRENT theta (include/mi355_carla.h): the policy net alone, forward only -- the twin of mi_ppo_values_idx, what the
// rollout buffers form their V-trace importance weights from.  M may exceed max_batch (the chunk loop is mi_ppo_fused_logp's).  Nothing of the training state is written.
int mi_ppo_logp_idx(void* h, void* stream, const float* states, const float* actions, const int* row_idx, long long n_rows, long long M, float* logp_out) {
    // (what needs no engine is checked before the handle is looked at)
    if (M < 1 || n_rows < 1) return mi_fail(MI_ERR_ARG, "mi_ppo_logp_idx: no rows (M < 1) or an empty table (n_rows < 1)");
    if (!states) return mi_fail(MI_ERR_ARG, "mi_ppo_logp_idx: missing buffers (states)");
    if (!actions) return mi_fail(MI_ERR_ARG, "mi_ppo_logp_idx: missing buffers (actions)");
    if (!logp_out) return mi_fail(MI_ERR_ARG, "mi_ppo_logp_idx: missing buffers (logp_out)");
    if (!row_idx && M > n_rows) return mi_fail(MI_ERR_ARG, "mi_ppo_logp_idx: without a row list the rows are 0 .. M - 1 of the table: M exceeds n_rows");
    PpoEngine* e = (PpoEngine*)h;
    if (!e) return mi_fail(MI_ERR_STATE, "mi_ppo_logp_idx: null handle");
    if (!fused_enabled(e)) return mi_fail(MI_ERR_SHAPE, "mi_ppo_logp_idx: needs the fused kernels (shape outside their range or MI355_PPO_FUSED=0)");
    PpoFusedParams q; fill_fused(e, q, states, 1);
    return mi_ppo_fused_logp((hipStream_t)stream, q, actions, row_idx, n_rows, M, logp_out, x3(e));
}

// precision of the engine's training forms (mi_ppo_train_step[_idx|_dp], the fused mi_ppo_forward_backward, mi_ppo_logp_old): MI_F32 (exact fp32, the default) or
// MI_BF16X3 (split-bf16 GEMM stages, ppo_fused.hip).  MI_BF16 has no PPO form; the split form exists only as fused kernels, so an engine that runs the per-layer
// path refuses it instead of training in fp32.  mi_ppo_predict and the rollout step stay exact fp32 in both modes.
int mi_ppo_set_precision(void* h, int dtype) {
    PpoEngine* e = (PpoEngine*)h;
    if (!e) return mi_fail(MI_ERR_STATE, "ppo engine: null handle");
    if (dtype != MI_F32 && dtype != MI_BF16X3) return mi_fail(MI_ERR_ARG, "mi_ppo_set_precision: MI_F32 or MI_BF16X3 (PPO has no bf16-storage mode)");
    if (dtype == MI_BF16X3 && !fused_enabled(e))
        return mi_fail(MI_ERR_SHAPE, "mi_ppo_set_precision: the split-bf16 mode needs the fused kernels (shape outside their range or MI355_PPO_FUSED=0)");
    e->precision = dtype;
    return MI_OK;
}

// Wide inputs (include/mi355_carla.h): which input widths the fused kernels take, and which layer-1 kernel serves the wide ones.  Routing only: the parameter
// layout (kin rows of W1, the last kin - din of them zero) is the same on every path, so the mode may change between two steps.
int mi_ppo_set_wide_inputs(void* h, int mode) {
    PpoEngine* e = (PpoEngine*)h;
    if (!e) return mi_fail(MI_ERR_STATE, "mi_ppo_set_wide_inputs: null handle");
    if (mode < 0 || mode > 2) return mi_fail(MI_ERR_ARG, "mi_ppo_set_wide_inputs: mode is 0 (fused range kin <= 96), 1 (kin <= 1024, the K-split layer 1) or 2 (kin <= 1024, ppo_l1_kernel)");
    if (x3(e) && mode == 0 && !mi_ppo_fused_shape_in_range(e->d.num_actions, e->d.h2, e->kin))
        return mi_fail(MI_ERR_SHAPE, "mi_ppo_set_wide_inputs: the engine is in the split-bf16 mode, which has no per-layer form (mi_ppo_set_precision(MI_F32) first)");
    e->wide = mode;
    return MI_OK;
}

int mi_ppo_wide_inputs(void* h) {
    PpoEngine* e = (PpoEngine*)h;
    if (!e) return mi_fail(MI_ERR_STATE, "mi_ppo_wide_inputs: null handle");
    return e->wide;
}

int mi_ppo_precision(void* h) {
    PpoEngine* e = (PpoEngine*)h;
    if (!e) return mi_fail(MI_ERR_STATE, "ppo engine: null handle");
    return e->precision;
}

// tf.train.AdamOptimizer over the 13 policy/ variables (ppo.py:143-144); alpha folds lr*lr_decay^episode and the bias correction
int mi_ppo_apply_adam(void* h, void* stream, float alpha, float beta1, float beta2, float epsilon) {
    PpoEngine* e = (PpoEngine*)h;
    if (!e) return mi_fail(MI_ERR_STATE, "ppo engine: null handle");
    if (!e->grads || !e->m || !e->v) return mi_fail(MI_ERR_STATE, "mi_ppo_apply_adam: engine created without optimiser buffers");
    return adam_prefix(e, stream, PPO_TENSORS, alpha, beta1, beta2, epsilon);
}

// Global-norm gradient clipping (tf.clip_by_global_norm in front of the optimiser; include/mi355_carla.h).  0: off, the default of a new engine.
int mi_ppo_set_max_grad_norm(void* h, float max_norm) {
    PpoEngine* e = (PpoEngine*)h;
    if (!e) return mi_fail(MI_ERR_STATE, "mi_ppo_set_max_grad_norm: null handle");
    // (what needs no engine is checked before the handle is looked at)
    if (!(max_norm >= 0.f)) return mi_fail(MI_ERR_ARG, "mi_ppo_set_max_grad_norm: max_norm is 0 (off), a positive float or +inf");
    e->max_grad_norm = max_norm;
    return MI_OK;
}

// Dual-clip PPO (include/mi355_carla.h; the definition is in ppo_fused.hip's head / loss kernel).  0: off, the default of a new engine.
int mi_ppo_set_dual_clip(void* h, float c) {
    PpoEngine* e = (PpoEngine*)h;
    if (!e) return mi_fail(MI_ERR_STATE, "mi_ppo_set_dual_clip: null handle");
    if (!(c == 0.f || c > 1.f)) return mi_fail(MI_ERR_ARG, "mi_ppo_set_dual_clip: c is 0 (off), a float > 1 or +inf");
    e->dual_clip = c == 0.f ? 0.f : c;                    // (-0.0 is stored as 0.0)
    return MI_OK;
}

float mi_ppo_dual_clip(void* h) {
    PpoEngine* e = (PpoEngine*)h;
    if (!e) { mi_fail(MI_ERR_STATE, "mi_ppo_dual_clip: null handle"); return -1.0f; }
    return e->dual_clip;
}

// The three loss coefficients of the descriptor, replaced on a live engine (include/mi355_carla.h): every later call reads e->d, so nothing else is to be done.
int mi_ppo_set_loss_coefs(void* h, float clip_eps, float value_scale, float entropy_scale) {
    PpoEngine* e = (PpoEngine*)h;
    if (!e) return mi_fail(MI_ERR_STATE, "mi_ppo_set_loss_coefs: null handle");
    const float fmax = 3.402823466e+38f;
    if (!(clip_eps > 0.f) || !(clip_eps <= fmax)) return mi_fail(MI_ERR_ARG, "mi_ppo_set_loss_coefs: clip_eps is a finite float > 0");
    if (!(value_scale >= 0.f) || !(value_scale <= fmax)) return mi_fail(MI_ERR_ARG, "mi_ppo_set_loss_coefs: value_scale is a finite float >= 0");
    if (!(entropy_scale >= 0.f) || !(entropy_scale <= fmax)) return mi_fail(MI_ERR_ARG, "mi_ppo_set_loss_coefs: entropy_scale is a finite float >= 0");
    e->d.clip_eps = clip_eps; e->d.value_scale = value_scale; e->d.entropy_scale = entropy_scale;
    return MI_OK;
}

int mi_ppo_loss_coefs(void* h, float* clip_eps, float* value_scale, float* entropy_scale) {
    PpoEngine* e = (PpoEngine*)h;
    if (!e) return mi_fail(MI_ERR_STATE, "mi_ppo_loss_coefs: null handle");
    if (!clip_eps || !value_scale || !entropy_scale) return mi_fail(MI_ERR_ARG, "mi_ppo_loss_coefs: missing outputs (clip_eps, value_scale, entropy_scale)");
    *clip_eps = e->d.clip_eps; *value_scale = e->d.value_scale; *entropy_scale = e->d.entropy_scale;
    return MI_OK;
}

float mi_ppo_max_grad_norm(void* h) {
    PpoEngine* e = (PpoEngine*)h;
    if (!e) { mi_fail(MI_ERR_STATE, "mi_ppo_max_grad_norm: null handle"); return -1.0f; }
    return e->max_grad_norm;
}

// the norm of the gradient buffer as it stands and the factor a limit of max_norm gives -> buffer 2; nothing else is written
int mi_ppo_grad_norm(void* h, void* stream, float max_norm) {
    PpoEngine* e = (PpoEngine*)h;
    if (!e) return mi_fail(MI_ERR_STATE, "mi_ppo_grad_norm: null handle");
    if (!(max_norm > 0.f)) return mi_fail(MI_ERR_ARG, "mi_ppo_grad_norm: max_norm is a positive float or +inf");
    if (!e->grads) return mi_fail(MI_ERR_STATE, "mi_ppo_grad_norm: engine created without a gradient buffer");
    CK(grad_sumsq(e, stream));
    return mi_grad_norm_finish((hipStream_t)stream, (const double*)e->at(e->gn_part), max_norm, (float*)e->at(e->clip));
}

}  // extern "C"
