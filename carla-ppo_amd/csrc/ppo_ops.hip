// ppo_ops.hip — wavefront-fused PPO kernels (gfx950, wave64):
//   clipped-surrogate / value / entropy losses with analytic gradients wrt the network heads,
//   Gaussian policy head (tanh squash, sample, clip), GAE reverse scan and advantage normalisation in fp64.
#include <cmath>

#include "common.hpp"
#include "mi_internal.hpp"
#include "mi355_carla.h"

using namespace mi;

namespace {

constexpr float HALF_LOG_2PI = 0.918938533204672741780329736406f;
constexpr int MAX_ACT = 8;

// ---------------------------------------------------------------------------------------------------
// PPO loss + head gradients (reference ppo.py:47,58-66,112-132).  One thread per sample.
//   u, u_old : [M,A] pre-tanh outputs of action_mean (policy / policy_old)     vraw : [M] value head output
//   mean = low + (tanh(u)+1)/2*(high-low) ; logp = sum_a -.5*((a-mean)/sigma)^2 - (.5log2pi + log sigma), sigma = exp(logstd)
//   ratio = exp(logp - logp_old) ; L_clip = mean(min(r*A, clip(r,1-e,1+e)*A)) ; L_v = vs*mean((V-R)^2) ; L_ent = es*sum_a(1.4189+log sigma)
//   loss = -L_clip + L_v - L_ent.   Outputs du [M,A], dv [M] (d loss / d head pre-activations, already / M),
//   per-block partials: [policy_sum, value_sq_sum, ratio_sum, dlogstd_0..A-1] -> finalised in ppo_loss_finalize_kernel.
// ---------------------------------------------------------------------------------------------------
constexpr int PPO_NPART = 3 + MAX_ACT;

__global__ __launch_bounds__(256) void ppo_loss_kernel(const float* __restrict__ u, const float* __restrict__ u_old,
                                                       const float* __restrict__ logstd, const float* __restrict__ logstd_old,
                                                       const float* __restrict__ vraw, const float* __restrict__ actions,
                                                       const float* __restrict__ returns, const float* __restrict__ adv,
                                                       const float* __restrict__ low, const float* __restrict__ high,
                                                       int M, int A, float clip_eps, float value_scale, float inv_m,
                                                       float* __restrict__ du, float* __restrict__ dv, float* __restrict__ partial) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    float vals[PPO_NPART];
#pragma unroll
    for (int k = 0; k < PPO_NPART; ++k) vals[k] = 0.f;
    if (i < M) {
        float logp = 0.f, logp_old = 0.f;
        float dlogp_dmean_scaled[MAX_ACT], zsq[MAX_ACT];
        for (int a = 0; a < A; ++a) {
            const float lo = low[a], hi = high[a];
            const float act = actions[(long long)i * A + a];
            const float t = tanhf(u[(long long)i * A + a]);
            const float mean = lo + ((t + 1.0f) * 0.5f) * (hi - lo);
            const float sigma = expf(logstd[a]);
            const float z = (act - mean) / sigma;
            logp += -0.5f * z * z - (HALF_LOG_2PI + logf(sigma));
            // d logp / d u = (act-mean)/sigma^2 * (hi-lo)/2 * (1 - t^2)
            dlogp_dmean_scaled[a] = (z / sigma) * (0.5f * (hi - lo)) * (1.0f - t * t);
            zsq[a] = z * z;
            const float to = tanhf(u_old[(long long)i * A + a]);
            const float mo = lo + ((to + 1.0f) * 0.5f) * (hi - lo);
            const float so = expf(logstd_old[a]);
            const float zo = (act - mo) / so;
            logp_old += -0.5f * zo * zo - (HALF_LOG_2PI + logf(so));
        }
        const float r = expf(logp - logp_old);
        const float ad = adv[i];
        const float rc = fminf(fmaxf(r, 1.0f - clip_eps), 1.0f + clip_eps);
        const float s1 = r * ad, s2 = rc * ad;
        vals[0] = fminf(s1, s2);
        // tf.minimum sends the gradient to the first argument when s1 <= s2 (ties included); the clipped branch has zero slope
        const float dr = (s1 <= s2) ? ad : 0.f;
        const float coef = -dr * r * inv_m;                       // d(-L_clip)/d logp
        for (int a = 0; a < A; ++a) {
            du[(long long)i * A + a] = coef * dlogp_dmean_scaled[a];
            vals[3 + a] = coef * (zsq[a] - 1.0f);                   // d(-L_clip)/d logstd_a   (d log sigma/d logstd = 1)
        }
        const float dvv = vraw[i] - returns[i];
        vals[1] = dvv * dvv;
        dv[i] = 2.0f * value_scale * dvv * inv_m;
        vals[2] = r;
    }
    __shared__ float red[4][PPO_NPART];
#pragma unroll
    for (int k = 0; k < PPO_NPART; ++k) {
        const float s = wave_sum(vals[k]);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][k] = s;
    }
    __syncthreads();
    if (threadIdx.x < PPO_NPART)
        partial[(long long)blockIdx.x * PPO_NPART + threadIdx.x] =
            (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
}

// losses[0..4] = policy_loss, value_loss, entropy_loss, loss, mean ratio ; dlogstd[a] (+)= grad.  Fixed block order.
__global__ void ppo_loss_finalize_kernel(const float* __restrict__ partial, int nblocks, const float* __restrict__ logstd, int A,
                                         float inv_m, float value_scale, float entropy_scale, float grad_scale,
                                         float* __restrict__ losses, float* __restrict__ dlogstd) {
    if (threadIdx.x != 0) return;
    float s[PPO_NPART];
    for (int k = 0; k < PPO_NPART; ++k) s[k] = 0.f;
    for (int b = 0; b < nblocks; ++b)
        for (int k = 0; k < 3 + A; ++k) s[k] += partial[(long long)b * PPO_NPART + k];
    float ent = 0.f;
    for (int a = 0; a < A; ++a) ent += 0.5f + HALF_LOG_2PI + logf(expf(logstd[a]));
    const float pl = s[0] * inv_m, vl = s[1] * inv_m * value_scale, el = ent * entropy_scale;
    losses[0] = pl; losses[1] = vl; losses[2] = el; losses[3] = -pl + vl - el; losses[4] = s[2] * inv_m;
    // entropy term is state independent: under data parallelism grad_scale = local_M / global_M shares it across ranks
    for (int a = 0; a < A; ++a) dlogstd[a] += s[3 + a] - entropy_scale * grad_scale;
}

// Gaussian head for predict() (reference ppo.py:47,58-62): mean from u; action = clip(mean + exp(logstd)*noise, low, high) or mean.
__global__ void policy_head_kernel(const float* __restrict__ u, const float* __restrict__ logstd, const float* __restrict__ noise,
                                   const float* __restrict__ low, const float* __restrict__ high, int M, int A, int greedy,
                                   float* __restrict__ action, float* __restrict__ mean_out) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= M * A) return;
    const int a = idx % A;
    const float lo = low[a], hi = high[a];
    const float mean = lo + ((tanhf(u[idx]) + 1.0f) * 0.5f) * (hi - lo);
    if (mean_out) mean_out[idx] = mean;
    float act = mean;
    if (!greedy) act = fminf(fmaxf(mean + expf(logstd[a]) * noise[idx], lo), hi);
    action[idx] = act;
}

// ---------------------------------------------------------------------------------------------------
// GAE (reference utils.py:45-50) in fp64 with the exact rounding sequence of numpy + scipy.signal.lfilter:
//   delta_t = r_t + ((1-done_t)*gamma)*V_{t+1} - V_t ;  A_t = delta_t + (gamma*lam)*A_{t+1}   (no FMA contraction)
// and returns = A + V ; A = (A - mean(A)) / (std(A) + 1e-8), population std (reference train.py:176-177).
// Every rounding sequence is spelled ONCE, in the helpers below; the dense kernels (one row = one trajectory) and the rollout finish kernels (one row or one
// episode segment of a ragged buffer) are shells around them, which is what makes a finished row or segment come out bit for bit as the dense kernels give it.
// Explicit __d*_rn calls or plain operators under -ffp-contract=off; no fma() here.
// ---------------------------------------------------------------------------------------------------
__device__ __forceinline__ double gae_delta(double r, double d, double vnext, double v, double gamma) {      // utils.py:45-48
    const double nonterm = __dsub_rn(1.0, d);
    return __dsub_rn(__dadd_rn(r, __dmul_rn(__dmul_rn(nonterm, gamma), vnext)), v);
}

// one step of lfilter's recurrence, walked from the last step to the first (utils.py:49-50): y = carry + delta ; carry = (gamma*lam) * y
__device__ __forceinline__ double gae_step(double& carry, double delta, double gl) {
    const double y = __dadd_rn(carry, delta);
    carry = __dmul_rn(gl, y);
    return y;
}

// One wave, L steps: v = the fp32 value slots (they widen to fp64 exactly), r / d = fp64 rewards / terminals of the first step, a = L doubles of LDS that hold the raw
// advantages on return.  The deltas do not depend on each other: all lanes form them; the recurrence is serial and lane 0 walks it in the dense kernel's order.
// SKIP_BEHIND_DONE: behind a terminal LAST step the bootstrap value is 0.0 and slot L is not read; without it slot L is read and the terminal flag masks it (the two
// differ in the sign of a zero and in what a NaN in slot L does).  FINAL with v_final != NULL (a TRUNCATED segment: the episode stopped without being terminal): the
// value behind the last step is *v_final and slot L is not read; the terminal flag of the last step masks it as it masks slot L.
// (the successor-value rule is gae_vnext, written once: the V-trace finish kernel forms its deltas by it too)
template <bool SKIP_BEHIND_DONE, bool FINAL>
__device__ __forceinline__ double gae_vnext(const float* v, const double* d, int t, int L, const float* v_final) {
    if (FINAL && v_final && t == L - 1) return (double)v_final[0];
    if (!SKIP_BEHIND_DONE || t < L - 1 || d[t] == 0.0) return (double)v[t + 1];
    return 0.0;
}
template <bool SKIP_BEHIND_DONE, bool FINAL = false>
__device__ __forceinline__ void finish_gae(double* a, const float* v, const double* r, const double* d, int L, double gamma, double gl, int lane, const float* v_final = nullptr) {
    for (int t = lane; t < L; t += WAVE) a[t] = gae_delta(r[t], d[t], gae_vnext<SKIP_BEHIND_DONE, FINAL>(v, d, t, L, v_final), (double)v[t], gamma);
    __syncthreads();
    if (lane == 0) {
        double carry = 0.0;
        for (int t = L - 1; t >= 0; --t) a[t] = gae_step(carry, a[t], gl);
    }
    __syncthreads();
}

// returns = A + V into the fp32 table (f64 -> f32 at the feed, ppo.py:108-109, round to nearest even) and the optional fp64 outputs; -> the wave's sum of A.
// tab / flat: the first step's position in the [num_envs (T + 1)] tables and in the [num_envs, T] arrays.  RAW_ALWAYS: adv_raw is not optional.
// dret: what the value is added to for the return -- the advantages themselves (nullptr: GAE), or the V-trace kernel's vs - V.
template <bool RAW_ALWAYS>
__device__ __forceinline__ double finish_returns(const double* a, const float* v, int L, int lane, long long tab, long long flat, float* tab_returns, double* returns,
                                                 double* adv_raw, const double* dret = nullptr) {
    if (!dret) dret = a;
    double s = 0.0;
    for (int t = lane; t < L; t += WAVE) {
        s += a[t];
        const double ret = dret[t] + (double)v[t];
        tab_returns[tab + t] = (float)ret;
        if (returns) returns[flat + t] = ret;
        if (RAW_ALWAYS || adv_raw) adv_raw[flat + t] = a[t];
    }
    return wave_sum_f64(s);
}

// sum over the wave's L values of (A - mean)^2, lane-strided from the first + the wave reduction (train.py:176-177's std, before the division)
__device__ __forceinline__ double sum_sq_dev(const double* a, double mean, int L, int lane) {
    double ss = 0.0;
    for (int t = lane; t < L; t += WAVE) { const double dd = a[t] - mean; ss += dd * dd; }
    return wave_sum_f64(ss);
}

// (A - mean) / (std + 1e-8) (train.py:177) into the fp32 table and the optional fp64 output
__device__ __forceinline__ void store_normalized(const double* a, double mean, double sd, int L, int lane, long long tab, long long flat, float* tab_adv, double* adv_norm) {
    for (int t = lane; t < L; t += WAVE) {
        const double an = (a[t] - mean) / (sd + 1e-8);
        tab_adv[tab + t] = (float)an;
        if (adv_norm) adv_norm[flat + t] = an;
    }
}

// the normalisation of one row or segment alone from its raw advantages and their sum s
__device__ __forceinline__ void finish_normalize(const double* a, double s, int L, int lane, long long tab, long long flat, float* tab_adv, double* adv_norm) {
    const double mean = s / (double)L;
    const double sd = sqrt(sum_sq_dev(a, mean, L, lane) / (double)L);
    store_normalized(a, mean, sd, L, lane, tab, flat, tab_adv, adv_norm);
}

// One thread per trajectory row; rows are independent (config C5 shards them across GPUs with no exchange).
__global__ void gae_scan_f64_kernel(const double* __restrict__ rewards, const double* __restrict__ values, const double* __restrict__ terminals,
                                    int R, int T, double gamma, double gl, double* __restrict__ adv) {
    const int row = blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= R) return;
    const double* r = rewards + (long long)row * T;
    const double* v = values + (long long)row * (T + 1);
    const double* d = terminals + (long long)row * T;
    double* o = adv + (long long)row * T;
    double carry = 0.0;
    for (int t = T - 1; t >= 0; --t) o[t] = gae_step(carry, gae_delta(r[t], d[t], v[t + 1], v[t], gamma), gl);
}

// returns = A + V, then the normalisation in place, per row.  One wave per row.  (It adds the values as it sums and normalises where it reads: its own loops.)
__global__ void adv_normalize_f64_kernel(double* __restrict__ adv, const double* __restrict__ values, int R, int T, double* __restrict__ returns) {
    const int row = blockIdx.x * (blockDim.x / WAVE) + threadIdx.x / WAVE;
    const int lane = threadIdx.x & 63;
    if (row >= R) return;
    double* a = adv + (long long)row * T;
    const double* v = values + (long long)row * (T + 1);
    double s = 0.0;
    for (int t = lane; t < T; t += WAVE) { s += a[t]; if (returns) returns[(long long)row * T + t] = a[t] + v[t]; }
    s = wave_sum_f64(s);
    const double mean = s / (double)T;
    const double sd = sqrt(sum_sq_dev(a, mean, T, lane) / (double)T);
    for (int t = lane; t < T; t += WAVE) a[t] = (a[t] - mean) / (sd + 1e-8);
}

}  // namespace

// ---------------------------------------------------------------------------------------------------
// mi_rollout_finish: GAE + returns + per-row normalisation of a RAGGED rollout buffer in one launch (utils.py:45-50, train.py:175-177 per row).  One wave (= one
// block) per row; row e has len[e] = L recorded steps in slots 0 .. L-1 of its T + 1 table slots and its bootstrap value in slot L.  The body is the helpers above,
// so a row comes out bit for bit as gae_scan_f64_kernel and adv_normalize_f64_kernel give it on that row alone.  Slots >= L and rows with L < 1 are not written.
// ---------------------------------------------------------------------------------------------------
namespace mi {
__global__ __launch_bounds__(64) void rollout_finish_kernel(const float* __restrict__ values, const double* __restrict__ rewards, const double* __restrict__ terminals,
                                                            const int* __restrict__ len, int T, double gamma, double gl, float* __restrict__ tab_returns,
                                                            float* __restrict__ tab_adv, double* __restrict__ adv_raw, double* __restrict__ returns, double* __restrict__ adv_norm) {
    __shared__ double a[MI_ROLLOUT_MAX_HORIZON];
    const int row = blockIdx.x, lane = threadIdx.x;
    const int L = min(len[row], T);                       // a length beyond the horizon cannot index past the row
    if (L < 1) return;
    const long long tab = (long long)row * (T + 1), flat = (long long)row * T;
    const float* v = values + tab;
    finish_gae<false>(a, v, rewards + flat, terminals + flat, L, gamma, gl, lane);
    const double s = finish_returns<false>(a, v, L, lane, tab, flat, tab_returns, returns, adv_raw);
    finish_normalize(a, s, L, lane, tab, flat, tab_adv, adv_norm);
}

// ---------------------------------------------------------------------------------------------------
// mi_rollout_finish_segments: the same finish for lanes that hold SEVERAL episodes (utils.py:45-50, train.py:175-177 per segment).  A segment is a run of n recorded
// steps inside one lane's step slots, given by the table row of its first slot; one wave (= one block) per segment runs the same helpers relative to that slot, so a
// segment comes out bit for bit as the dense kernels give it on that segment alone.  A segment whose last step is terminal bootstraps from 0.0 and does not
// read the slot behind it (the next episode's first value, or a stale one).  The deltas need n <= T doubles of LDS: the launch sizes the dynamic LDS by T, not by
// MI_ROLLOUT_MAX_HORIZON, so that short horizons keep many segments resident per CU.  A descriptor that does not lie inside one lane's step slots is not executed.
// NORM = 1 (normalisation over the batch): this kernel leaves the raw advantages in adv_raw and the segment's sum in part[seg]; the kernels below do the rest in a
// fixed order: partials in lane-strided segment order by one wave, no floating-point atomics.
// ---------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool rollout_seg_decode(int r, int n, int num_envs, int T, long long& flat) {
    if (n < 1 || r < 0) return false;
    const int env = r / (T + 1), slot = r - env * (T + 1);
    if (env >= num_envs || (long long)slot + n > T) return false;      // (a first slot of T, the lane's bootstrap slot, fails here for every n >= 1)
    flat = (long long)env * T + slot;
    return true;
}

template <int NORM>
__global__ __launch_bounds__(64) void rollout_finish_seg_kernel(const float* __restrict__ values, const double* __restrict__ rewards, const double* __restrict__ terminals,
                                                                const int* __restrict__ seg_row, const int* __restrict__ seg_len, int num_envs, int T, double gamma, double gl,
                                                                float* __restrict__ tab_returns, float* __restrict__ tab_adv, double* __restrict__ adv_raw,
                                                                double* __restrict__ returns, double* __restrict__ adv_norm, double* __restrict__ part) {
    extern __shared__ double seg_a[];                      // T doubles
    double* a = seg_a;
    const int seg = blockIdx.x, lane = threadIdx.x;
    const int L = seg_len[seg];
    const long long tab = seg_row[seg];
    long long flat;
    if (!rollout_seg_decode((int)tab, L, num_envs, T, flat)) {
        if (NORM && lane == 0) part[seg] = 0.0;            // adds nothing to the batch sum
        return;
    }
    const float* v = values + tab;
    finish_gae<true>(a, v, rewards + flat, terminals + flat, L, gamma, gl, lane);
    const double s = finish_returns<NORM != 0>(a, v, L, lane, tab, flat, tab_returns, returns, adv_raw);
    if (NORM) {
        if (lane == 0) part[seg] = s;
        return;
    }
    finish_normalize(a, s, L, lane, tab, flat, tab_adv, adv_norm);
}

// mi_rollout_finish_segments_boot: rollout_finish_seg_kernel with a per-segment bootstrap source.  seg_boot[seg] == 0: that kernel's rule.  seg_boot[seg] != 0 (the
// segment was TRUNCATED: its episode stopped without being terminal and the lane went on with a reset observation): the value behind the last step is
// final_values[row of the last step] -- the value of the episode's final observation, which is no step of the lane and so has no slot in `values` -- and the slot
// behind the segment, the next episode's first value or a stale one, is not read.  The same helpers: a truncated segment comes out bit for bit as the dense kernels
// give it on [v_0 .. v_{L-1}, v_final].  A kernel of its own, so that the one above stays the code it was.  NORM = 1: as above, the same kernels follow.
template <int NORM>
__global__ __launch_bounds__(64) void rollout_finish_seg_boot_kernel(const float* __restrict__ values, const float* __restrict__ final_values, const double* __restrict__ rewards,
                                                                     const double* __restrict__ terminals, const int* __restrict__ seg_row, const int* __restrict__ seg_len,
                                                                     const int* __restrict__ seg_boot, int num_envs, int T, double gamma, double gl,
                                                                     float* __restrict__ tab_returns, float* __restrict__ tab_adv, double* __restrict__ adv_raw,
                                                                     double* __restrict__ returns, double* __restrict__ adv_norm, double* __restrict__ part) {
    extern __shared__ double seg_boot_a[];                 // T doubles
    double* a = seg_boot_a;
    const int seg = blockIdx.x, lane = threadIdx.x;
    const int L = seg_len[seg];
    const long long tab = seg_row[seg];
    long long flat;
    if (!rollout_seg_decode((int)tab, L, num_envs, T, flat)) {
        if (NORM && lane == 0) part[seg] = 0.0;
        return;
    }
    const float* v = values + tab;
    const float* v_final = seg_boot[seg] != 0 ? final_values + tab + (L - 1) : nullptr;      // (inside the table: the segment lies inside one lane's step slots)
    finish_gae<true, true>(a, v, rewards + flat, terminals + flat, L, gamma, gl, lane, v_final);
    const double s = finish_returns<NORM != 0>(a, v, L, lane, tab, flat, tab_returns, returns, adv_raw);
    if (NORM) {
        if (lane == 0) part[seg] = s;
        return;
    }
    finish_normalize(a, s, L, lane, tab, flat, tab_adv, adv_norm);
}

// One wave: the n_seg partials in lane-strided segment order + the wave reduction.  STAGE 0: stat[0] = mean of all steps of all executed segments (their count from the
// descriptors, by the same test); STAGE 1: stat[1] = population std from the partial sums of squared deviations.
template <int STAGE>
__global__ __launch_bounds__(64) void rollout_seg_reduce_kernel(const double* __restrict__ part, const int* __restrict__ seg_row, const int* __restrict__ seg_len, int n_seg,
                                                                int num_envs, int T, double* __restrict__ stat) {
    const int lane = threadIdx.x;
    double s = 0.0, cnt = 0.0;                             // the count is exact in fp64 (at most 2^22 steps)
    for (int i = lane; i < n_seg; i += WAVE) {
        long long flat;
        s += part[i];
        if (rollout_seg_decode(seg_row[i], seg_len[i], num_envs, T, flat)) cnt += (double)seg_len[i];
    }
    s = wave_sum_f64(s);
    cnt = wave_sum_f64(cnt);
    if (lane == 0) stat[STAGE] = cnt < 1.0 ? 0.0 : (STAGE == 0 ? s / cnt : sqrt(s / cnt));
}

// PASS 0: part[seg] = sum over the segment of (A - mean)^2; PASS 1: (A - mean) / (std + 1e-8) into the fp32 table and adv_norm.  Both read the raw advantages
// rollout_finish_seg_kernel<1> left in adv_raw.
template <int PASS>
__global__ __launch_bounds__(64) void rollout_seg_norm_kernel(const double* __restrict__ adv_raw, const int* __restrict__ seg_row, const int* __restrict__ seg_len, int num_envs,
                                                              int T, const double* __restrict__ stat, double* __restrict__ part, float* __restrict__ tab_adv,
                                                              double* __restrict__ adv_norm) {
    const int seg = blockIdx.x, lane = threadIdx.x;
    const int L = seg_len[seg];
    const long long tab = seg_row[seg];
    long long flat;
    if (!rollout_seg_decode((int)tab, L, num_envs, T, flat)) {
        if (PASS == 0 && lane == 0) part[seg] = 0.0;
        return;
    }
    const double* a = adv_raw + flat;
    const double mean = stat[0];
    if (PASS == 0) {
        const double ss = sum_sq_dev(a, mean, L, lane);
        if (lane == 0) part[seg] = ss;
    } else {
        store_normalized(a, mean, stat[1], L, lane, tab, flat, tab_adv, adv_norm);
    }
}

// ---------------------------------------------------------------------------------------------------
// mi_rollout_finish_vtrace: the finish of rollout_finish_seg_kernel / rollout_finish_seg_boot_kernel with V-trace's truncated importance weights (Espeholt et al.
// 2018) on the recurrence.  One wave (= one block) per segment; the dynamic LDS holds two arrays of T doubles.  All lanes form, for t < L, the delta of step t --
// gae_delta on the successor value of gae_vnext: READ_BEHIND = true is mi_rollout_finish's rule (the slot behind a terminal last step is read and masked), false the
// segment kernels' (0.0 there, the slot is not read); a truncated segment (seg_boot) takes final_values under either -- and the weight
// w_t = exp((double)lp_now[t] - (double)lp_old[t]).  Lane 0 walks t = L - 1 .. 0 with Dn = 0.0, explicit roundings, no fma:
//     cw = min(c_bar, w_t), rw = min(rho_bar, w_t)          (as w > bar ? bar : w: a NaN weight is not masked)
//     A_t = gl Dn + delta_t                                  the policy advantage delta_t + gamma lam (vs_{t+1} - V_{t+1})
//     D_t = (gl cw) Dn + rw delta_t                          vs_t - V_t;  Dn = D_t
// and the returns are D_t + V_t, the V-trace value target.  The weight of step t does not multiply A_t: PPO's surrogate applies the ratio itself.  As in the GAE
// kernels the recurrence is not cut at a terminal inside a segment: segments end at their terminal.
// THE GAE IDENTITY: with w_t = 1 and both bars >= 1, cw = rw = 1.0 and every product with them is exact, so D_t = A_t = gl A_{t+1} + delta_t in gae_step's
// roundings: the kernel stores what the GAE kernel of the same successor rule stores, bit for bit.  The sums, the returns and the normalisation are the helpers'.
// ---------------------------------------------------------------------------------------------------
template <int NORM, bool READ_BEHIND>
__global__ __launch_bounds__(64) void rollout_finish_vtrace_kernel(const float* __restrict__ values, const float* __restrict__ lp_now, const float* __restrict__ lp_old,
                                                                   const float* __restrict__ final_values, const double* __restrict__ rewards,
                                                                   const double* __restrict__ terminals, const int* __restrict__ seg_row, const int* __restrict__ seg_len,
                                                                   const int* __restrict__ seg_boot, int num_envs, int T, double gamma, double gl, double rho_bar, double c_bar,
                                                                   float* __restrict__ tab_returns, float* __restrict__ tab_adv, double* __restrict__ adv_raw,
                                                                   double* __restrict__ returns, double* __restrict__ adv_norm, double* __restrict__ weights_out,
                                                                   double* __restrict__ part) {
    extern __shared__ double seg_vt[];                     // 2 T doubles: delta -> A | w -> D
    double* a = seg_vt;
    double* w = seg_vt + T;
    const int seg = blockIdx.x, lane = threadIdx.x;
    const int L = seg_len[seg];
    const long long tab = seg_row[seg];
    long long flat;
    if (!rollout_seg_decode((int)tab, L, num_envs, T, flat)) {
        if (NORM && lane == 0) part[seg] = 0.0;            // adds nothing to the batch sum
        return;
    }
    const float* v = values + tab;
    const double* r = rewards + flat; const double* d = terminals + flat;
    const float* v_final = (seg_boot && seg_boot[seg] != 0) ? final_values + tab + (L - 1) : nullptr;
    for (int t = lane; t < L; t += WAVE) {
        a[t] = gae_delta(r[t], d[t], gae_vnext<!READ_BEHIND, true>(v, d, t, L, v_final), (double)v[t], gamma);
        const double wt = exp((double)lp_now[tab + t] - (double)lp_old[tab + t]);
        w[t] = wt;
        if (weights_out) weights_out[flat + t] = wt;
    }
    __syncthreads();
    if (lane == 0) {
        double Dn = 0.0;
        for (int t = L - 1; t >= 0; --t) {
            const double wt = w[t], delta = a[t];
            const double cw = wt > c_bar ? c_bar : wt;
            const double rw = wt > rho_bar ? rho_bar : wt;
            a[t] = __dadd_rn(__dmul_rn(gl, Dn), delta);
            Dn = __dadd_rn(__dmul_rn(__dmul_rn(gl, cw), Dn), __dmul_rn(rw, delta));
            w[t] = Dn;
        }
    }
    __syncthreads();
    const double s = finish_returns<NORM != 0>(a, v, L, lane, tab, flat, tab_returns, returns, adv_raw, w);
    if (NORM) {
        if (lane == 0) part[seg] = s;
        return;
    }
    finish_normalize(a, s, L, lane, tab, flat, tab_adv, adv_norm);
}

// ---------------------------------------------------------------------------------------------------
// mi_rollout_scale_rewards: the rewards of one collection divided by the running standard deviation of the discounted return (baselines' VecNormalize, at the
// granularity of an update), in front of the finish kernels above.  Lane e has L = min(len[e], T) recorded steps; G[e,t] = c * gamma + r[e,t] with c = carry[e] at t = 0,
// c = G[e,t] behind a step that neither is terminal nor truncated and 0.0 behind one that is.  Four launches, fp64, no atomics, every sum in a fixed order:
//   rollout_reward_scan_kernel    one wave (= one block) per lane, the shape of finish_gae: all lanes stage the rewards and the reset flags in LDS (T doubles + T bytes:
//                                 the launch sizes the dynamic LDS by T), lane 0 walks the recurrence, all lanes store G and sum it lane-strided: part[e] = the lane's sum
//   rollout_reward_dev_kernel     one wave per lane: the batch mean from the partials (every block adds them alike, in lane-strided order, so all blocks hold the same
//                                 bits; block 0 leaves n_b and m_b in stat), then part2[e] = the lane's sum of (G - m_b)^2
//   rollout_reward_merge_kernel   one wave: M2_b from part2 in lane-strided order, the Chan / Welford merge into state (merge = 1) and den = sqrt(var + epsilon)
//   rollout_reward_scale_kernel   one wave per lane: rewards_out = min(max(r / den, -clip), clip)
// Slots >= L are neither read nor written; a lane with L < 1 adds 0.0 and keeps its carry.
// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void rollout_reward_scan_kernel(const double* __restrict__ rewards, const double* __restrict__ terminals, const unsigned char* __restrict__ truncs,
                                                                 const int* __restrict__ len, int T, double gamma, double* __restrict__ carry, double* __restrict__ g_out,
                                                                 double* __restrict__ part) {
    extern __shared__ double scan_g[];                     // T doubles, then T bytes of reset flags
    double* g = scan_g;
    unsigned char* cut = reinterpret_cast<unsigned char*>(scan_g + T);
    const int row = blockIdx.x, lane = threadIdx.x;
    const int L = min(len[row], T);                        // a length beyond the horizon cannot index past the row
    if (L < 1) {
        if (lane == 0) part[row] = 0.0;                    // adds nothing to the batch sum
        return;
    }
    const long long flat = (long long)row * T;
    for (int t = lane; t < L; t += WAVE) {
        g[t] = rewards[flat + t];
        cut[t] = (terminals[flat + t] != 0.0 || (truncs && truncs[flat + t])) ? 1 : 0;
    }
    __syncthreads();
    if (lane == 0) {
        double c = carry[row];
        for (int t = 0; t < L; ++t) {
            const double y = __dadd_rn(__dmul_rn(c, gamma), g[t]);      // one multiply, one add
            g[t] = y;
            c = cut[t] ? 0.0 : y;
        }
        carry[row] = c;
    }
    __syncthreads();
    double s = 0.0;
    for (int t = lane; t < L; t += WAVE) { s += g[t]; g_out[flat + t] = g[t]; }
    s = wave_sum_f64(s);
    if (lane == 0) part[row] = s;
}

// -> the sum of the num_envs partials in lane-strided order + the wave reduction: the same bits in every wave that calls it
__device__ __forceinline__ double reward_partials_sum(const double* part, int num_envs, int lane) {
    double s = 0.0;
    for (int i = lane; i < num_envs; i += WAVE) s += part[i];
    return wave_sum_f64(s);
}

__global__ __launch_bounds__(64) void rollout_reward_dev_kernel(const double* __restrict__ g_out, const int* __restrict__ len, int num_envs, int T,
                                                                const double* __restrict__ part, double* __restrict__ part2, double* __restrict__ stat) {
    const int row = blockIdx.x, lane = threadIdx.x;
    double cnt = 0.0;                                      // the count is exact in fp64 (at most 2^22 steps)
    for (int i = lane; i < num_envs; i += WAVE) cnt += (double)max(min(len[i], T), 0);
    cnt = wave_sum_f64(cnt);
    const double s = reward_partials_sum(part, num_envs, lane);
    const double mean = cnt < 1.0 ? 0.0 : s / cnt;
    if (row == 0 && lane == 0) { stat[0] = cnt; stat[1] = mean; }
    const int L = min(len[row], T);
    const double ss = L < 1 ? 0.0 : sum_sq_dev(g_out + (long long)row * T, mean, L, lane);
    if (lane == 0) part2[row] = ss;
}

// state = {count, mean, M2, den}.  merge = 0 (frozen statistics) and an empty batch leave count, mean and M2 as they were.
__global__ __launch_bounds__(64) void rollout_reward_merge_kernel(const double* __restrict__ part2, const double* __restrict__ stat, int num_envs, int merge, double epsilon,
                                                                  double* __restrict__ state) {
    const int lane = threadIdx.x;
    const double m2_b = reward_partials_sum(part2, num_envs, lane);
    if (lane != 0) return;
    double count = state[0];
    const double n_b = stat[0];
    if (merge && n_b >= 1.0) {
        const double mean = state[1], delta = stat[1] - mean, n_new = count + n_b;
        state[1] = mean + delta * n_b / n_new;
        state[2] = state[2] + (m2_b + delta * delta * count * n_b / n_new);
        state[0] = count = n_new;
    }
    const double var = count > 0.0 ? state[2] / count : 1.0;
    state[3] = sqrt(var + epsilon);
}

__global__ __launch_bounds__(64) void rollout_reward_scale_kernel(const double* __restrict__ rewards, const int* __restrict__ len, int T, const double* __restrict__ state,
                                                                  double clip, double* __restrict__ rewards_out) {
    const int row = blockIdx.x, lane = threadIdx.x;
    const int L = min(len[row], T);
    const long long flat = (long long)row * T;
    const double den = state[3];
    for (int t = lane; t < L; t += WAVE) rewards_out[flat + t] = fmin(fmax(rewards[flat + t] / den, -clip), clip);
}

// ---------------------------------------------------------------------------------------------------
// mi_rollout_obs_stats: the running per-column moments behind observation normalisation (the other half of baselines' VecNormalize), in the style of the pass above:
// fp64, ordered sums, no atomics.  The n rows row_idx[i] of the fp32 table tab [n_table_rows][din] (a row outside the table is skipped and does not count) are cut into
// nb = ceil(n / chunk) blocks of `chunk` consecutive list entries -- chunk = max(32, ceil(n / 256)), a function of n alone, so two runs add the same terms in the same
// order --; thread t of a block owns the columns t, t + 128, .. and walks its block's rows in list order (neighbouring threads read neighbouring floats of a row).
//   rollout_obs_sum_kernel     part[b][j] = the block's column sum, cnt[b] = its rows inside the table, clampc[b][j] = how many of its entries obs_normalize() -- the
//                              normalise kernel's expression -- puts at +-clip under the mean32 / inv32 the collection was normalised with
//   rollout_obs_dev_kernel     the batch mean of column j from the partials in block order (every block adds them alike: the same bits everywhere; block 0 leaves
//                              them and the count in scratch), then part2[b][j] = the block's sum of (x - m_b[j])^2
//   rollout_obs_merge_kernel   one block: M2_b[j] from part2 in block order, the Chan / Welford merge into state = {count, mean[din], M2[din]} (merge = 1) and the
//                              derived fp32 mean32[j] / inv32[j] = 1 / sqrt(M2[j] / count + epsilon)  (columns below first_col: 0 / 1)
//                              A batch with an entry that is not finite (some batch mean is not finite) is not merged at all: state stays bitwise as it was
// ---------------------------------------------------------------------------------------------------
constexpr int OBS_THREADS = 128;

__global__ __launch_bounds__(OBS_THREADS) void rollout_obs_sum_kernel(const float* __restrict__ tab, long long n_table_rows, const int* __restrict__ row_idx, long long n, int din,
                                                                      int chunk, const float* __restrict__ obs_mean, const float* __restrict__ obs_inv_std, float clip,
                                                                      double* __restrict__ part, double* __restrict__ clampc, double* __restrict__ cnt) {
    const long long b = blockIdx.x, lo = b * chunk, hi = min(lo + (long long)chunk, n);
    for (int j = threadIdx.x; j < din; j += OBS_THREADS) {
        const float m32 = obs_mean[j], inv32 = obs_inv_std[j];
        double s = 0.0, c = 0.0, k = 0.0;
        for (long long i = lo; i < hi; ++i) {
            const long long r = row_idx[i];
            if (r < 0 || r >= n_table_rows) continue;
            const float x = tab[r * din + j];
            s += (double)x;
            k += 1.0;
            if (fabsf(obs_normalize(x, m32, inv32, clip)) == clip) c += 1.0;
        }
        part[b * din + j] = s;
        clampc[b * din + j] = c;
        if (j == 0) cnt[b] = k;
    }
}

__global__ __launch_bounds__(OBS_THREADS) void rollout_obs_dev_kernel(const float* __restrict__ tab, long long n_table_rows, const int* __restrict__ row_idx, long long n, int din,
                                                                      int chunk, int nb, const double* __restrict__ part, const double* __restrict__ cnt,
                                                                      double* __restrict__ part2, double* __restrict__ bmean, double* __restrict__ bcount) {
    const long long b = blockIdx.x, lo = b * chunk, hi = min(lo + (long long)chunk, n);
    for (int j = threadIdx.x; j < din; j += OBS_THREADS) {
        double tot = 0.0, k = 0.0;                         // (the count is exact in fp64)
        for (int bb = 0; bb < nb; ++bb) { tot += part[(long long)bb * din + j]; k += cnt[bb]; }
        const double mean = k < 1.0 ? 0.0 : tot / k;
        if (b == 0) {
            bmean[j] = mean;
            if (j == 0) bcount[0] = k;
        }
        double ss = 0.0;
        for (long long i = lo; i < hi; ++i) {
            const long long r = row_idx[i];
            if (r < 0 || r >= n_table_rows) continue;
            const double d = (double)tab[r * din + j] - mean;
            ss += d * d;
        }
        part2[b * din + j] = ss;
    }
}

// nb = 0 (an empty list): nothing is merged and the batch figures are 0.  merge = 0, an empty batch and a batch that is not finite leave state bitwise as it was.
__global__ __launch_bounds__(OBS_THREADS) void rollout_obs_merge_kernel(int din, int nb, int first_col, int merge, double epsilon, const double* __restrict__ part2,
                                                                        const double* __restrict__ clampc, const double* __restrict__ bmean,
                                                                        const double* __restrict__ bcount, double* __restrict__ state, float* __restrict__ obs_mean,
                                                                        float* __restrict__ obs_inv_std, double* __restrict__ batch_out) {
    const double count = state[0], n_b = nb > 0 ? bcount[0] : 0.0;
    // a batch with an entry that is not finite is not merged, in any column: it would make mean / M2 NaN for good.  A column's batch mean is finite exactly when all
    // its entries are (fewer than 2^31 fp32 terms cannot overflow an fp64 sum); the caller sees the refusal in batch_out's means.
    int fin = 1;                                           // (each wave looks at every column, a lane at every 64th, and votes: no LDS)
    for (int j = threadIdx.x & (WAVE - 1); j < din && nb > 0; j += WAVE) fin &= isfinite(bmean[j]) ? 1 : 0;
    const bool finite = __all(fin);
    __syncthreads();                                       // every thread holds the old count before thread 0 stores the new one
    const bool do_merge = merge && n_b >= 1.0 && finite;
    const double n_new = do_merge ? count + n_b : count;
    for (int j = threadIdx.x; j < din; j += OBS_THREADS) {
        double m2_b = 0.0, cl = 0.0;
        for (int bb = 0; bb < nb; ++bb) { m2_b += part2[(long long)bb * din + j]; cl += clampc[(long long)bb * din + j]; }
        const double m_b = nb > 0 ? bmean[j] : 0.0;
        double mean = state[1 + j], m2 = state[1 + din + j];
        if (do_merge) {
            const double delta = m_b - mean;
            mean = mean + delta * n_b / n_new;
            m2 = m2 + (m2_b + delta * delta * count * n_b / n_new);
            state[1 + j] = mean;
            state[1 + din + j] = m2;
        }
        const double var = n_new > 0.0 ? m2 / n_new : 1.0;
        const double inv = 1.0 / sqrt(var + epsilon);
        const bool normalized = j >= first_col;
        obs_mean[j] = normalized ? (float)mean : 0.f;
        obs_inv_std[j] = normalized ? (float)inv : 1.f;
        batch_out[j] = m_b;
        batch_out[din + j] = m2_b;
        batch_out[2 * din + j] = cl;
    }
    if (threadIdx.x == 0 && do_merge) state[0] = n_new;
}
}  // namespace mi

// ---------------------------------------------------------------------------------------------------
// mi_ppo_value_clip_stats: the sums behind the value-clipping diagnostics over M rows row_idx[m] (clamped) of three fp32 tables -- v = V under the current parameters
// (the value_out table of mi_ppo_update_stats_idx), vo = the value recorded at collection time, ret = the return -- formed in double from the fp32 inputs:
//   v_c = min(max(v, vo - eps), vo + eps), l_u = (v - ret)^2, l_c = (v_c - ret)^2: terms 1, |v - vo| > eps, max(l_u, l_c), l_c > l_u
// One thread per sample.  Ordered reduction as in ppo_update_stats_head_kernel, no atomics: an xor tree of shuffles inside a wave, the four waves' sums in LDS added in
// wave order and stored as this block's row of `scratch`; ppo_value_clip_reduce_kernel adds the rows in block order.  Rows that row_idx does not name are not read.
// ---------------------------------------------------------------------------------------------------
namespace mi {
constexpr int VC_NSTATS = MI_PPO_N_VCLIP_STATS;
__global__ __launch_bounds__(256) void ppo_value_clip_stats_kernel(const float* __restrict__ values_new, const float* __restrict__ old_values, const float* __restrict__ returns,
                                                                   const int* __restrict__ row_idx, int n_rows, int M, double eps, double* __restrict__ scratch) {
    __shared__ double swave[4][VC_NSTATS];
    const int tid = threadIdx.x, m = blockIdx.x * 256 + tid, wave = tid >> 6;
    double term[VC_NSTATS];
#pragma unroll
    for (int k = 0; k < VC_NSTATS; ++k) term[k] = 0.0;
    if (m < M) {
        const long long mr = min(max(row_idx[m], 0), n_rows - 1);
        const double v = (double)values_new[mr], vo = (double)old_values[mr], ret = (double)returns[mr];
        const double vc = fmin(fmax(v, vo - eps), vo + eps);
        const double lu = (v - ret) * (v - ret), lc = (vc - ret) * (vc - ret);
        term[0] = 1.0; term[1] = fabs(v - vo) > eps ? 1.0 : 0.0; term[2] = fmax(lu, lc); term[3] = lc > lu ? 1.0 : 0.0;
    }
#pragma unroll
    for (int k = 0; k < VC_NSTATS; ++k) {
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) term[k] += __shfl_xor(term[k], o, 64);
    }
    if ((tid & 63) == 0) {
#pragma unroll
        for (int k = 0; k < VC_NSTATS; ++k) swave[wave][k] = term[k];
    }
    __syncthreads();
    if (tid < VC_NSTATS) scratch[(long long)blockIdx.x * VC_NSTATS + tid] = ((swave[0][tid] + swave[1][tid]) + swave[2][tid]) + swave[3][tid];
}

// one wave: lane k adds column k of the block rows in block order, then stores (accumulate 0) or adds to (1) stats[k]
__global__ __launch_bounds__(64) void ppo_value_clip_reduce_kernel(const double* __restrict__ scratch, int n_blocks, int accumulate, double* __restrict__ stats) {
    const int k = threadIdx.x;
    if (k >= VC_NSTATS) return;
    double sum = 0.0;
    for (int b = 0; b < n_blocks; ++b) sum += scratch[(long long)b * VC_NSTATS + k];
    stats[k] = accumulate ? stats[k] + sum : sum;
}
}  // namespace mi

// ---------------------------------------------------------------------------------------------------
// mi_ppo_minibatch_advantages: the advantages of one epoch normalised PER MINIBATCH (SB3 normalize_advantage, CleanRL norm_adv; no counterpart in train.py), between the
// finish kernels above, which leave the raw advantages in fp64 [num_envs, T], and the SGD steps, which gather their advantage from an fp32 table by row.  Minibatch b is
// perm[b batch_size .. min((b + 1) batch_size, n)), table rows e (T + 1) + t; an entry that names no step slot (rollout_seg_decode's rule for a one-step segment: row < 0,
// lane >= num_envs, slot T) is skipped: it does not count and nothing is stored for it.  One launch, one block of four waves per minibatch, fp64, three passes over the
// minibatch's positions, each of which reads perm and the gathered doubles from global memory again (a minibatch can be the whole collection: no LDS is sized by it):
//   1  c = the counted entries, mean = sum(a) / c        2  ss = sum((a - mean)^2), std = c - ddof >= 1 ? sqrt(ss / (c - ddof)) : 0
//   3  tab_adv_out[row] = (float)((a - mean) / (std + 1e-8))      (store_normalized's true division)
// Every sum in ONE order, no atomics: thread i adds positions i, i + 256, .. from the first, wave_sum_f64 inside each wave, the four waves' partials through LDS and
// added in wave order by thread 0, which hands the result to the block.  stats[b] = {c, mean, std}; {0, 0, 0} and no store for a minibatch without a counted entry.
// ---------------------------------------------------------------------------------------------------
namespace mi {
constexpr int MBA_THREADS = 256;
static_assert(MBA_THREADS == 4 * WAVE, "mba_block_sum adds four waves' partials");

// -> the block's sum of v, the same bits in every thread.  red: MBA_THREADS / WAVE + 1 doubles of LDS; every thread of the block calls it.
__device__ __forceinline__ double mba_block_sum(double v, double* red, int tid) {
    v = wave_sum_f64(v);
    if ((tid & (WAVE - 1)) == 0) red[tid / WAVE] = v;
    __syncthreads();
    if (tid == 0) red[MBA_THREADS / WAVE] = ((red[0] + red[1]) + red[2]) + red[3];
    __syncthreads();
    const double s = red[MBA_THREADS / WAVE];
    __syncthreads();                                       // (the next call stores into red)
    return s;
}

__global__ __launch_bounds__(MBA_THREADS) void ppo_minibatch_adv_kernel(const double* __restrict__ adv_raw, const int* __restrict__ perm, int n, int batch_size, int num_envs,
                                                                        int T, int ddof, float* __restrict__ tab_adv_out, double* __restrict__ stats) {
    __shared__ double red[MBA_THREADS / WAVE + 1];
    const int tid = threadIdx.x;
    const long long first = (long long)blockIdx.x * batch_size;
    const long long left = (long long)n - first;           // >= 1: the grid is ceil(n / batch_size) blocks
    const int m = left < batch_size ? (int)left : batch_size;
    const int* rows = perm + first;
    long long flat;
    double s = 0.0, cnt = 0.0;                             // the count is exact in fp64
    for (int i = tid; i < m; i += MBA_THREADS)
        if (rollout_seg_decode(rows[i], 1, num_envs, T, flat)) { s += adv_raw[flat]; cnt += 1.0; }
    const double c = mba_block_sum(cnt, red, tid);
    s = mba_block_sum(s, red, tid);
    double* out = stats + 3LL * blockIdx.x;
    if (c < 1.0) {                                         // (the same c in every thread: the whole block leaves)
        if (tid < 3) out[tid] = 0.0;
        return;
    }
    const double mean = s / c;
    double ss = 0.0;
    for (int i = tid; i < m; i += MBA_THREADS)
        if (rollout_seg_decode(rows[i], 1, num_envs, T, flat)) { const double dd = adv_raw[flat] - mean; ss += dd * dd; }
    ss = mba_block_sum(ss, red, tid);
    const double dof = c - (double)ddof;
    const double sd = dof >= 1.0 ? sqrt(ss / dof) : 0.0;
    for (int i = tid; i < m; i += MBA_THREADS)
        if (rollout_seg_decode(rows[i], 1, num_envs, T, flat)) tab_adv_out[rows[i]] = (float)((adv_raw[flat] - mean) / (sd + 1e-8));
    if (tid == 0) { out[0] = c; out[1] = mean; out[2] = sd; }
}
}  // namespace mi

namespace {
__global__ __launch_bounds__(256) void relu_grad_kernel(const float* __restrict__ g, const float* __restrict__ h, long long n, float* __restrict__ out) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = h[i] > 0.f ? g[i] : 0.f;
}
}  // namespace

extern "C" {

int mi_ppo_loss_blocks(int M) { return (M + 255) / 256; }
int mi_ppo_loss_partial_floats(int M) { return mi_ppo_loss_blocks(M) * PPO_NPART; }

int mi_ppo_loss_fwd_bwd(void* stream, const float* u, const float* u_old, const float* logstd, const float* logstd_old, const float* vraw,
                        const float* actions, const float* returns, const float* advantage, const float* low, const float* high,
                        int M, int A, float clip_eps, float value_scale, float entropy_scale, float inv_m, float grad_scale,
                        float* du, float* dv, float* partial, float* losses5, float* dlogstd) {
    if (A < 1 || A > MAX_ACT) return mi_fail(MI_ERR_ARG, "mi_ppo_loss_fwd_bwd: 1 <= num_actions <= 8");
    if (M < 1) return mi_fail(MI_ERR_ARG, "mi_ppo_loss_fwd_bwd: empty minibatch");
    const int nb = mi_ppo_loss_blocks(M);
    hipLaunchKernelGGL(ppo_loss_kernel, dim3(nb), dim3(256), 0, (hipStream_t)stream, u, u_old, logstd, logstd_old, vraw, actions, returns,
                       advantage, low, high, M, A, clip_eps, value_scale, inv_m, du, dv, partial);
    hipLaunchKernelGGL(ppo_loss_finalize_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, partial, nb, logstd, A, inv_m, value_scale,
                       entropy_scale, grad_scale, losses5, dlogstd);
    return mi_check_launch("ppo_loss");
}

long long mi_ppo_value_clip_stats_scratch_doubles(int M) { return (long long)MI_PPO_N_VCLIP_STATS * (M < 1 ? 1 : (M + 255) / 256); }

int mi_ppo_value_clip_stats(void* stream, const float* values_new, const float* old_values, const float* returns, const int* row_idx, int n_rows, int M,
                            float clip_range_vf, int accumulate, double* scratch, double* stats) {
    if (M < 1 || n_rows < 1) return mi_fail(MI_ERR_ARG, "mi_ppo_value_clip_stats: empty input (M >= 1, n_rows >= 1)");
    if (!values_new || !old_values || !returns || !row_idx || !scratch || !stats) return mi_fail(MI_ERR_ARG, "mi_ppo_value_clip_stats: missing buffers");
    if (!(clip_range_vf > 0.f)) return mi_fail(MI_ERR_ARG, "mi_ppo_value_clip_stats: clip_range_vf is a positive float or +inf");
    if (accumulate != 0 && accumulate != 1) return mi_fail(MI_ERR_ARG, "mi_ppo_value_clip_stats: accumulate is 0 (store the sums) or 1 (add them to stats)");
    const int nb = (M + 255) / 256;
    hipLaunchKernelGGL(ppo_value_clip_stats_kernel, dim3(nb), dim3(256), 0, (hipStream_t)stream, values_new, old_values, returns, row_idx, n_rows, M, (double)clip_range_vf, scratch);
    hipLaunchKernelGGL(ppo_value_clip_reduce_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (const double*)scratch, nb, accumulate, stats);
    return mi_check_launch("ppo_value_clip_stats");
}

// stats: {count, mean, std} per minibatch
long long mi_ppo_minibatch_advantages_stats_doubles(int n, int batch_size) {
    return (n < 1 || batch_size < 1) ? -1 : 3LL * (((long long)n + batch_size - 1) / batch_size);
}

// adv_raw fp64 [num_envs, T], perm int32 [n] table rows, tab_adv_out fp32 [num_envs (T + 1)], stats fp64 [ceil(n / batch_size), 3] (all device).  Every check runs
// before the launch.
#define MBA_FAIL(text) return mi_fail(MI_ERR_ARG, "mi_ppo_minibatch_advantages: " text)
int mi_ppo_minibatch_advantages(void* stream, const double* adv_raw, const int* perm, int n, int batch_size, int num_envs, int T, int ddof, float* tab_adv_out,
                                double* stats) {
    if (!adv_raw) MBA_FAIL("adv_raw is missing");
    if (!perm) MBA_FAIL("perm is missing");
    if (!tab_adv_out) MBA_FAIL("tab_adv_out is missing");
    if (!stats) MBA_FAIL("stats is missing");
    if (n < 1) MBA_FAIL("n: perm holds at least one entry (n >= 1)");
    if (batch_size < 1) MBA_FAIL("batch_size >= 1");
    if (num_envs < 1 || num_envs > MI_ROLLOUT_MAX_ENVS) MBA_FAIL("num_envs outside [1, MI_ROLLOUT_MAX_ENVS]");
    if (T < 1 || T > MI_ROLLOUT_MAX_HORIZON) MBA_FAIL("T outside [1, MI_ROLLOUT_MAX_HORIZON]");
    if (ddof != 0 && ddof != 1) MBA_FAIL("ddof is 0 (population std) or 1 (sample std)");
    const long long n_mb = ((long long)n + batch_size - 1) / batch_size;
    hipLaunchKernelGGL(ppo_minibatch_adv_kernel, dim3((unsigned)n_mb), dim3(MBA_THREADS), 0, (hipStream_t)stream, adv_raw, perm, n, batch_size, num_envs, T, ddof,
                       tab_adv_out, stats);
    return mi_check_launch("ppo_minibatch_advantages");
}
#undef MBA_FAIL

int mi_policy_head(void* stream, const float* u, const float* logstd, const float* noise, const float* low, const float* high,
                   int M, int A, int greedy, float* action, float* mean_out) {
    if (!greedy && !noise) return mi_fail(MI_ERR_ARG, "mi_policy_head: sampling needs noise");
    hipLaunchKernelGGL(policy_head_kernel, dim3((M * A + 255) / 256), dim3(256), 0, (hipStream_t)stream, u, logstd, noise, low, high, M, A, greedy, action, mean_out);
    return mi_check_launch("policy_head");
}

// rewards [R,T], values [R,T+1] (last column = bootstrap), terminals [R,T] (0/1), all fp64 -> adv [R,T]
// build_mlp trunk of the policy / value network as OP-level calls (SURVEY 8b names; the engines use the fused forms of ppo_fused.hip): utils.py:25-28 with
// hidden sizes (H1, H2) and ReLU on both layers (ppo.py:42-44,51-53).  Exact fp32 (the same dense kernels the engine's unfused path runs).
//   fwd: h1 = relu(x W1 + b1) [M, H1], h2 = relu(h1 W2 + b2) [M, H2]                       W1 [din, H1], W2 [H1, H2] (tf.layers.dense kernels)
//   bwd: given g2 = dL/dh2 (post-activation) [M, H2]: dW2 += h1^T (g2 . relu'(h2)), db2 += column sums, dW1 += x^T dh1, db1 += ..., with
//        dh1 = ((g2 . relu'(h2)) W2^T) . relu'(h1); scratch: M * (H1 + H2) floats.  The gradient wrt x is not produced (nothing upstream of the state trains).
int mi_mlp_policy_fwd(void* stream, const float* x, int M, int din, const float* W1, const float* b1, int H1, const float* W2, const float* b2, int H2, float* h1, float* h2) {
    if (!x || !W1 || !b1 || !W2 || !b2 || !h1 || !h2 || M < 1 || din < 1 || H1 < 1 || H2 < 1) return mi_fail(MI_ERR_ARG, "mi_mlp_policy_fwd: missing buffers or empty shape");
    if (din % 4 != 0 || H1 % 4 != 0 || H2 % 4 != 0) return mi_fail(MI_ERR_SHAPE, "mi_mlp_policy_fwd: din, H1, H2 must be multiples of 4 (16-byte rows; pad the state with zero columns as the engine does)");
    int rc = mi_gemm_bias_act(stream, MI_F32, x, M, din, W1, 0, H1, b1, 1, nullptr, h1, 1, 1);
    if (rc != MI_OK) return rc;
    return mi_gemm_bias_act(stream, MI_F32, h1, M, H1, W2, 0, H2, b2, 1, nullptr, h2, 1, 1);
}
int mi_mlp_policy_bwd(void* stream, const float* x, int M, int din, const float* W2, int H1, int H2, const float* h1, const float* h2, const float* g2,
                      float* dW1, float* db1, float* dW2, float* db2, float* scratch) {
    if (!x || !W2 || !h1 || !h2 || !g2 || !dW1 || !db1 || !dW2 || !db2 || !scratch || M < 1) return mi_fail(MI_ERR_ARG, "mi_mlp_policy_bwd: missing buffers or empty shape");
    float* g2m = scratch; float* dh1 = scratch + (long long)M * H2;
    if (din % 4 != 0 || H1 % 4 != 0 || H2 % 4 != 0) return mi_fail(MI_ERR_SHAPE, "mi_mlp_policy_bwd: din, H1, H2 must be multiples of 4 (16-byte rows; pad the state with zero columns as the engine does)");
    {
        const long long n = (long long)M * H2;
        hipLaunchKernelGGL(relu_grad_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, g2, h2, n, g2m);
        const int rc0 = mi_check_launch("relu_grad_kernel");
        if (rc0 != MI_OK) return rc0;
    }
    int rc = MI_OK;
    rc = mi_colsum(stream, MI_F32, g2m, M, H2, db2);
    if (rc == MI_OK) rc = mi_gemm_wgrad(stream, MI_F32, h1, g2m, M, H1, H2, dW2);
    if (rc == MI_OK) rc = mi_gemm_bias_act(stream, MI_F32, g2m, M, H2, W2, 1, H1, nullptr, 0, h1, dh1, 1, 1);      // x W^T with the ReluGrad mask of h1
    if (rc == MI_OK) rc = mi_colsum(stream, MI_F32, dh1, M, H1, db1);
    if (rc == MI_OK) rc = mi_gemm_wgrad(stream, MI_F32, x, dh1, M, din, H1, dW1);
    return rc;
}

int mi_gae_scan(void* stream, const double* rewards, const double* values, const double* terminals, int R, int T, double gamma, double lam, double* adv) {
    if (R < 1 || T < 1) return mi_fail(MI_ERR_ARG, "mi_gae_scan: empty input");
    hipLaunchKernelGGL(gae_scan_f64_kernel, dim3((R + 63) / 64), dim3(64), 0, (hipStream_t)stream, rewards, values, terminals, R, T, gamma, gamma * lam, adv);
    return mi_check_launch("gae_scan");
}

int mi_adv_normalize(void* stream, double* adv, const double* values, int R, int T, double* returns) {
    if (R < 1 || T < 1) return mi_fail(MI_ERR_ARG, "mi_adv_normalize: empty input");
    hipLaunchKernelGGL(adv_normalize_f64_kernel, dim3((R + 3) / 4), dim3(256), 0, (hipStream_t)stream, adv, values, R, T, returns);
    return mi_check_launch("adv_normalize");
}

// rewards / terminals [num_envs, T] fp64, values: the fp32 table [num_envs (T + 1)], len [num_envs] int32 (all device) -> fp32 tables and optional fp64 [num_envs, T] outputs
int mi_rollout_finish(void* stream, const float* tab_values, const double* rewards, const double* terminals, const int* len, int num_envs, int T, double gamma, double lam,
                      float* tab_returns, float* tab_advantages, double* adv_raw, double* returns, double* adv_norm) {
    if (!tab_values || !rewards || !terminals || !len || !tab_returns || !tab_advantages) return mi_fail(MI_ERR_ARG, "mi_rollout_finish: missing buffers");
    if (num_envs < 1 || T < 1) return mi_fail(MI_ERR_ARG, "mi_rollout_finish: empty input (num_envs >= 1, T >= 1)");
    if (T > MI_ROLLOUT_MAX_HORIZON) return mi_fail(MI_ERR_ARG, "mi_rollout_finish: the horizon exceeds MI_ROLLOUT_MAX_HORIZON");
    hipLaunchKernelGGL(rollout_finish_kernel, dim3(num_envs), dim3(64), 0, (hipStream_t)stream, tab_values, rewards, terminals, len, T, gamma, gamma * lam,
                       tab_returns, tab_advantages, adv_raw, returns, adv_norm);
    return mi_check_launch("rollout_finish");
}

// scratch of normalize = 1: per-segment sums | per-segment sums of squared deviations | mean, std
long long mi_rollout_finish_segments_scratch_doubles(int n_seg) { return n_seg < 1 ? -1 : 2LL * n_seg + 2; }

// mi_rollout_finish with segment descriptors in place of len: seg_row / seg_len int32 [n_seg] (device).  One body for mi_rollout_finish_segments (boot = false: its
// kernel, its launches) and mi_rollout_finish_segments_boot (the first kernel takes the per-segment bootstrap source; the batch normalisation behind it is the same).
#define SEG_FAIL(text) return mi_fail(MI_ERR_ARG, boot ? "mi_rollout_finish_segments_boot: " text : "mi_rollout_finish_segments: " text)
static int finish_segments(bool boot, void* stream, const float* tab_values, const double* rewards, const double* terminals, const int* seg_row, const int* seg_len, int n_seg,
                           int num_envs, int T, double gamma, double lam, int normalize, double* scratch, float* tab_returns, float* tab_advantages, double* adv_raw,
                           double* returns, double* adv_norm, const float* tab_final_values, const int* seg_boot) {
    if (!tab_values || !rewards || !terminals || !seg_row || !seg_len || !tab_returns || !tab_advantages) SEG_FAIL("missing buffers");
    if (boot && (!tab_final_values || !seg_boot)) SEG_FAIL("missing buffers (tab_final_values, seg_boot)");
    if (n_seg < 1 || num_envs < 1 || T < 1) SEG_FAIL("empty input (n_seg >= 1, num_envs >= 1, T >= 1)");
    if (T > MI_ROLLOUT_MAX_HORIZON) SEG_FAIL("the horizon exceeds MI_ROLLOUT_MAX_HORIZON");
    if (normalize != 0 && normalize != 1) SEG_FAIL("normalize is 0 (per segment) or 1 (per batch)");
    if (normalize == 1 && (!scratch || !adv_raw)) SEG_FAIL("normalize = 1 needs scratch and adv_raw (missing buffers)");
    hipStream_t st = (hipStream_t)stream;
    const size_t lds = (size_t)T * sizeof(double);
    const double gl = gamma * lam;
    double* part = normalize ? scratch : nullptr;
    if (boot) {
        if (normalize == 0)
            hipLaunchKernelGGL(rollout_finish_seg_boot_kernel<0>, dim3(n_seg), dim3(64), lds, st, tab_values, tab_final_values, rewards, terminals, seg_row, seg_len, seg_boot,
                               num_envs, T, gamma, gl, tab_returns, tab_advantages, adv_raw, returns, adv_norm, part);
        else
            hipLaunchKernelGGL(rollout_finish_seg_boot_kernel<1>, dim3(n_seg), dim3(64), lds, st, tab_values, tab_final_values, rewards, terminals, seg_row, seg_len, seg_boot,
                               num_envs, T, gamma, gl, tab_returns, tab_advantages, adv_raw, returns, adv_norm, part);
    } else if (normalize == 0) {
        hipLaunchKernelGGL(rollout_finish_seg_kernel<0>, dim3(n_seg), dim3(64), lds, st, tab_values, rewards, terminals, seg_row, seg_len, num_envs, T, gamma, gl, tab_returns,
                           tab_advantages, adv_raw, returns, adv_norm, part);
    } else {
        hipLaunchKernelGGL(rollout_finish_seg_kernel<1>, dim3(n_seg), dim3(64), lds, st, tab_values, rewards, terminals, seg_row, seg_len, num_envs, T, gamma, gl, tab_returns,
                           tab_advantages, adv_raw, returns, adv_norm, part);
    }
    if (normalize == 0) return mi_check_launch(boot ? "rollout_finish_seg_boot" : "rollout_finish_seg");
    double* part2 = scratch + n_seg;
    double* stat = scratch + 2LL * n_seg;
    hipLaunchKernelGGL(rollout_seg_reduce_kernel<0>, dim3(1), dim3(64), 0, st, part, seg_row, seg_len, n_seg, num_envs, T, stat);
    hipLaunchKernelGGL(rollout_seg_norm_kernel<0>, dim3(n_seg), dim3(64), 0, st, adv_raw, seg_row, seg_len, num_envs, T, stat, part2, tab_advantages, adv_norm);
    hipLaunchKernelGGL(rollout_seg_reduce_kernel<1>, dim3(1), dim3(64), 0, st, part2, seg_row, seg_len, n_seg, num_envs, T, stat);
    hipLaunchKernelGGL(rollout_seg_norm_kernel<1>, dim3(n_seg), dim3(64), 0, st, adv_raw, seg_row, seg_len, num_envs, T, stat, part2, tab_advantages, adv_norm);
    return mi_check_launch(boot ? "rollout_finish_seg_boot (batch normalisation)" : "rollout_finish_seg (batch normalisation)");
}
#undef SEG_FAIL

int mi_rollout_finish_segments(void* stream, const float* tab_values, const double* rewards, const double* terminals, const int* seg_row, const int* seg_len, int n_seg,
                               int num_envs, int T, double gamma, double lam, int normalize, double* scratch, float* tab_returns, float* tab_advantages, double* adv_raw,
                               double* returns, double* adv_norm) {
    return finish_segments(false, stream, tab_values, rewards, terminals, seg_row, seg_len, n_seg, num_envs, T, gamma, lam, normalize, scratch, tab_returns, tab_advantages,
                           adv_raw, returns, adv_norm, nullptr, nullptr);
}

// seg_boot int32 [n_seg] (device): != 0 = the segment was truncated and bootstraps from tab_final_values[row of its last step] (fp32 [num_envs (T + 1)])
int mi_rollout_finish_segments_boot(void* stream, const float* tab_values, const double* rewards, const double* terminals, const int* seg_row, const int* seg_len, int n_seg,
                                    int num_envs, int T, double gamma, double lam, int normalize, double* scratch, float* tab_returns, float* tab_advantages, double* adv_raw,
                                    double* returns, double* adv_norm, const float* tab_final_values, const int* seg_boot) {
    return finish_segments(true, stream, tab_values, rewards, terminals, seg_row, seg_len, n_seg, num_envs, T, gamma, lam, normalize, scratch, tab_returns, tab_advantages,
                           adv_raw, returns, adv_norm, tab_final_values, seg_boot);
}

// The V-trace finish (include/mi355_carla.h): rollout_finish_vtrace_kernel, and with normalize = 1 the four launches of the batch normalisation behind it.
// tab_logp_now / tab_logp_old fp32 [num_envs (T + 1)]; tab_final_values / seg_boot both or neither; weights_out fp64 [num_envs, T] or NULL.  Every check runs
// before the first launch.
#define VT_FAIL(text) return mi_fail(MI_ERR_ARG, "mi_rollout_finish_vtrace: " text)
int mi_rollout_finish_vtrace(void* stream, const float* tab_values, const float* tab_logp_now, const float* tab_logp_old, const double* rewards, const double* terminals,
                             const int* seg_row, const int* seg_len, int n_seg, int num_envs, int T, double gamma, double lam, double rho_bar, double c_bar,
                             int read_behind_done, int normalize, double* scratch, float* tab_returns, float* tab_advantages, double* adv_raw, double* returns,
                             double* adv_norm, double* weights_out, const float* tab_final_values, const int* seg_boot) {
    if (!tab_values || !tab_logp_now || !tab_logp_old || !rewards || !terminals || !seg_row || !seg_len || !tab_returns || !tab_advantages) VT_FAIL("missing buffers");
    if ((tab_final_values != nullptr) != (seg_boot != nullptr)) VT_FAIL("tab_final_values and seg_boot come together or are both NULL");
    if (n_seg < 1 || num_envs < 1 || T < 1) VT_FAIL("empty input (n_seg >= 1, num_envs >= 1, T >= 1)");
    if (T > MI_ROLLOUT_MAX_HORIZON) VT_FAIL("the horizon exceeds MI_ROLLOUT_MAX_HORIZON");
    if (!(rho_bar > 0.0)) VT_FAIL("rho_bar is a positive value (+inf: never truncates)");
    if (!(c_bar >= 0.0)) VT_FAIL("c_bar is a value >= 0 (+inf: never truncates)");
    if (read_behind_done != 0 && read_behind_done != 1) VT_FAIL("read_behind_done is 0 (the segment kernels' successor rule) or 1 (mi_rollout_finish's)");
    if (normalize != 0 && normalize != 1) VT_FAIL("normalize is 0 (per segment) or 1 (per batch)");
    if (normalize == 1 && (!scratch || !adv_raw)) VT_FAIL("normalize = 1 needs scratch and adv_raw (missing buffers)");
    hipStream_t st = (hipStream_t)stream;
    const size_t lds = 2 * (size_t)T * sizeof(double);
    const double gl = gamma * lam;
    double* part = normalize ? scratch : nullptr;
#define VT_LAUNCH(NORM, RB) hipLaunchKernelGGL((rollout_finish_vtrace_kernel<NORM, RB>), dim3(n_seg), dim3(64), lds, st, tab_values, tab_logp_now, tab_logp_old, \
        tab_final_values, rewards, terminals, seg_row, seg_len, seg_boot, num_envs, T, gamma, gl, rho_bar, c_bar, tab_returns, tab_advantages, adv_raw, returns, adv_norm, \
        weights_out, part)
    if (normalize == 0) { if (read_behind_done) VT_LAUNCH(0, true); else VT_LAUNCH(0, false); }
    else { if (read_behind_done) VT_LAUNCH(1, true); else VT_LAUNCH(1, false); }
#undef VT_LAUNCH
    if (normalize == 0) return mi_check_launch("rollout_finish_vtrace");
    double* part2 = scratch + n_seg;
    double* stat = scratch + 2LL * n_seg;
    hipLaunchKernelGGL(rollout_seg_reduce_kernel<0>, dim3(1), dim3(64), 0, st, part, seg_row, seg_len, n_seg, num_envs, T, stat);
    hipLaunchKernelGGL(rollout_seg_norm_kernel<0>, dim3(n_seg), dim3(64), 0, st, adv_raw, seg_row, seg_len, num_envs, T, stat, part2, tab_advantages, adv_norm);
    hipLaunchKernelGGL(rollout_seg_reduce_kernel<1>, dim3(1), dim3(64), 0, st, part2, seg_row, seg_len, n_seg, num_envs, T, stat);
    hipLaunchKernelGGL(rollout_seg_norm_kernel<1>, dim3(n_seg), dim3(64), 0, st, adv_raw, seg_row, seg_len, num_envs, T, stat, part2, tab_advantages, adv_norm);
    return mi_check_launch("rollout_finish_vtrace (batch normalisation)");
}
#undef VT_FAIL

// scratch: per-lane sums of G | per-lane sums of squared deviations | n_b, m_b
long long mi_rollout_scale_rewards_scratch_doubles(int num_envs) { return num_envs < 1 ? -1 : 2LL * num_envs + 2; }

// rewards / terminals fp64 [num_envs, T], truncs uint8 [num_envs, T] or NULL, len int32 [num_envs], state [4], carry [num_envs] (all device) -> g_out / rewards_out fp64
// [num_envs, T], state and carry advanced.  Every check runs before the first launch.
#define SCALE_FAIL(text) return mi_fail(MI_ERR_ARG, "mi_rollout_scale_rewards: " text)
int mi_rollout_scale_rewards(void* stream, const double* rewards, const double* terminals, const unsigned char* truncs, const int* len, int num_envs, int T, double gamma,
                             double epsilon, double clip, int merge, double* state, double* carry, double* scratch, double* g_out, double* rewards_out) {
    if (!rewards || !terminals || !len || !state || !carry || !scratch || !g_out || !rewards_out) SCALE_FAIL("missing buffers");
    if (num_envs < 1 || T < 1) SCALE_FAIL("empty input (num_envs >= 1, T >= 1)");
    if (T > MI_ROLLOUT_MAX_HORIZON) SCALE_FAIL("the horizon exceeds MI_ROLLOUT_MAX_HORIZON");
    if (num_envs > MI_ROLLOUT_MAX_ENVS) SCALE_FAIL("num_envs exceeds MI_ROLLOUT_MAX_ENVS");
    if (!(gamma >= 0.0 && gamma <= 1.0)) SCALE_FAIL("gamma outside [0, 1]");
    if (!std::isfinite(epsilon) || epsilon < 0.0) SCALE_FAIL("epsilon is a finite value >= 0");
    if (!(clip > 0.0)) SCALE_FAIL("clip is a positive value (+inf: never clamp)");
    if (merge != 0 && merge != 1) SCALE_FAIL("merge is 0 (frozen statistics) or 1");
    hipStream_t st = (hipStream_t)stream;
    double* part = scratch;
    double* part2 = scratch + num_envs;
    double* stat = scratch + 2LL * num_envs;
    const size_t lds = (size_t)T * (sizeof(double) + 1);
    hipLaunchKernelGGL(rollout_reward_scan_kernel, dim3(num_envs), dim3(64), lds, st, rewards, terminals, truncs, len, T, gamma, carry, g_out, part);
    hipLaunchKernelGGL(rollout_reward_dev_kernel, dim3(num_envs), dim3(64), 0, st, g_out, len, num_envs, T, part, part2, stat);
    hipLaunchKernelGGL(rollout_reward_merge_kernel, dim3(1), dim3(64), 0, st, part2, stat, num_envs, merge, epsilon, state);
    hipLaunchKernelGGL(rollout_reward_scale_kernel, dim3(num_envs), dim3(64), 0, st, rewards, len, T, state, clip, rewards_out);
    return mi_check_launch("rollout_scale_rewards");
}
#undef SCALE_FAIL

// rows per block of the moments pass and the number of blocks: functions of n alone
static int obs_stats_chunk(long long n) { const long long c = (n + 255) / 256; return (int)(c < 32 ? 32 : c); }
static int obs_stats_blocks(long long n) { const int c = obs_stats_chunk(n); return (int)((n + c - 1) / c); }

// scratch: column sums | squared deviations | clamped counts, [nb][din] each | rows per block [nb] | batch mean [din] | batch count
long long mi_rollout_obs_stats_scratch_doubles(long long n, int din) {
    if (n < 1 || din < 1 || n > 0x7fffffffLL) return -1;
    const long long nb = obs_stats_blocks(n);
    return 3 * nb * din + nb + din + 1;
}

// Every check runs before the first launch.
#define OBS_FAIL(text) return mi_fail(MI_ERR_ARG, "mi_rollout_obs_stats: " text)
int mi_rollout_obs_stats(void* stream, const float* tab_raw_states, long long n_table_rows, const int* row_idx, long long n, int din, int first_col, int merge,
                         double epsilon, float clip, double* state, float* obs_mean, float* obs_inv_std, double* scratch, double* batch_out) {
    if (!state || !obs_mean || !obs_inv_std || !batch_out) OBS_FAIL("missing buffers");
    if (n < 0 || n > 0x7fffffffLL) OBS_FAIL("n is the length of the row list, 0 <= n < 2^31 (0: derive only)");
    if (n > 0 && (!tab_raw_states || !row_idx || !scratch)) OBS_FAIL("missing buffers");
    if (din < 1 || (n > 0 && n_table_rows < 1)) OBS_FAIL("empty input (din >= 1, n_table_rows >= 1)");
    if (first_col < 0 || first_col > din) OBS_FAIL("first_col outside [0, din]");
    if (merge != 0 && merge != 1) OBS_FAIL("merge is 0 (frozen statistics) or 1");
    if (!std::isfinite(epsilon) || epsilon < 0.0) OBS_FAIL("epsilon is a finite value >= 0");
    if (!(clip > 0.f)) OBS_FAIL("clip is a positive value (+inf: never clamp)");
    hipStream_t st = (hipStream_t)stream;
    const int nb = n > 0 ? obs_stats_blocks(n) : 0, chunk = n > 0 ? obs_stats_chunk(n) : 0;
    double* part = scratch;
    double* part2 = nb ? part + (long long)nb * din : nullptr;
    double* clampc = nb ? part2 + (long long)nb * din : nullptr;
    double* cnt = nb ? clampc + (long long)nb * din : nullptr;
    double* bmean = nb ? cnt + nb : nullptr;
    double* bcount = nb ? bmean + din : nullptr;
    if (nb) {
        hipLaunchKernelGGL(rollout_obs_sum_kernel, dim3(nb), dim3(OBS_THREADS), 0, st, tab_raw_states, n_table_rows, row_idx, n, din, chunk, obs_mean, obs_inv_std, clip,
                           part, clampc, cnt);
        hipLaunchKernelGGL(rollout_obs_dev_kernel, dim3(nb), dim3(OBS_THREADS), 0, st, tab_raw_states, n_table_rows, row_idx, n, din, chunk, nb, part, cnt, part2, bmean,
                           bcount);
    }
    hipLaunchKernelGGL(rollout_obs_merge_kernel, dim3(1), dim3(OBS_THREADS), 0, st, din, nb, first_col, merge, epsilon, part2, clampc, bmean, bcount, state, obs_mean,
                       obs_inv_std, batch_out);
    return mi_check_launch("rollout_obs_stats");
}
#undef OBS_FAIL

}  // extern "C"
