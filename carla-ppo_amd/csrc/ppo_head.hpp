// ppo_head.hpp — the pieces the head-level kernels of ppo_fused.hip share, each written once.  All __device__ __forceinline__: a kernel is its helpers inlined, the
// __shared__ arrays go in as pointers (plain ones: the address space is inferred through the inlined call, no flat access; pf_head_sums alone wants them typed), and
// the order of every floating-point operation is the helper's, whoever calls it.  That is what the bit-for-bit contracts between the kernels rest on (pf_mean_libm / pf_logp_term_libm below).
//
//   the 16-byte form (32 samples per block, 8 lanes per sample, h2 rows in registers from the first request to the dh2 stores):
//     pf_head_rows, pf_stage_request / pf_stage_commit, pf_head_sums, pf_fast_tanh, pf_block_partials, pf_head_dh2
//         -> ppo_head_loss_body (8 instantiations, and 8 with DEMO: the step with a demonstration term), ppo_head_clone_kernel (4)
//   the strided form (columns j = part, part + TPS, .. straight from memory; libm):
//     pf_head_sums_strided, pf_mean_libm, pf_logp_term_libm
//         -> ppo_predict_head_kernel (4), ppo_update_stats_head_kernel (2), ppo_kl_stats_head_kernel (2), ppo_values_head_kernel (1: the value half of the sums
//            alone), ppo_logp_head_kernel (2: the policy half alone); the two libm spellings also in the loss body's
//            old-policy block, whose sums stay there (from LDS, in the strided order)
//     pf_ordered_block_sum, ppo_stats_reduce_kernel
//         -> the two statistics kernels and the launch behind each
#pragma once
#include "common.hpp"
#include "ppo_fused.hpp"

namespace mi {

constexpr float PF_HALF_LOG_2PI = 0.918938533204672741780329736406f;
constexpr int PF_MAX_ACT = 8;
constexpr int PF_NPART = 3 + 2 * PF_MAX_ACT;             // per loss block: policy sum, value sq sum, ratio sum, dlogstd[A], action-mean sums [A]
constexpr int PF_H2MAX = 320;                             // head kernels staged in LDS: H2 <= 320 (the reference: 300)
constexpr int PF_NV = (PF_H2MAX / 4 + 7) / 8;             // float4 pieces per thread and h2 row (10)
constexpr int PF_NSV = (PF_H2MAX + 255) / 256;            // value head kernel: staged floats per thread

// this thread's 16-byte pieces f = part, part + 8, .. of sample m's h2 rows of net 0 (hp) and net 1 (hv), all requested before anything is used.  VAL = false
// (the policy-only clone step) loads no value row and zeroes hv.  A template flag, not a run-time test: a uniform branch between the two nets' loads makes the
// compiler wait for each pair of pieces before it requests the next (profiles/r34_behaviour_cloning.md section 1: + 6.8 % on the step at M = 32)
template <int NV, bool VAL>
__device__ __forceinline__ void pf_head_rows(const PpoFusedParams& q, int m, bool mok, int part, f32x4 (&hp)[NV], f32x4 (&hv)[NV]) {
    const int H2 = q.H2, nf = H2 >> 2;                    // float4 per row (H2 % 4 == 0)
    const float* __restrict__ h2p = q.h2; const float* __restrict__ h2v = q.h2 + (long long)q.M * H2;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int f = part + 8 * i;
        const bool ok = mok && f < nf;
        hp[i] = ok ? *(const f32x4*)(h2p + (long long)m * H2 + 4 * f) : f32x4{0.f, 0.f, 0.f, 0.f};
        if constexpr (VAL) hv[i] = ok ? *(const f32x4*)(h2v + (long long)m * H2 + 4 * f) : f32x4{0.f, 0.f, 0.f, 0.f};
        else hv[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
}

// head kernels -> LDS through registers, as a pair: pf_stage_request brings the policy head Wm, with OLD the old policy's Wmo (only if old_net: without a cached
// log pi_old) and with VAL the value head Wv into registers, pf_stage_commit stores them.  The caller's per-sample scalar gathers stand between the two, so that
// all requests are in flight together.  Without OLD there is no sWo (nullptr); without VAL sWv is filled with zeros.
template <int NA> struct PfHeadStage { float m[(PF_H2MAX * NA + 255) / 256], o[(PF_H2MAX * NA + 255) / 256], v[PF_NSV]; };
template <int NA, bool OLD, bool VAL>
__device__ __forceinline__ void pf_stage_request(const PpoFusedParams& q, int tid, bool old_net, PfHeadStage<NA>& st) {
    const int A = q.A, H2 = q.H2;
    const float* __restrict__ Wm = q.theta + q.off[4]; const float* __restrict__ Wmo = q.theta_old + q.off[4]; const float* __restrict__ Wv = q.theta + q.off[11];
#pragma unroll
    for (int i = 0; i < (PF_H2MAX * NA + 255) / 256; ++i) {
        const int x = tid + 256 * i;
        st.m[i] = x < H2 * A ? Wm[x] : 0.f;
        if constexpr (OLD) st.o[i] = (old_net && x < H2 * A) ? Wmo[x] : 0.f;
    }
#pragma unroll
    for (int i = 0; i < PF_NSV; ++i) { const int x = tid + 256 * i; st.v[i] = (VAL && x < H2) ? Wv[x] : 0.f; }
}
template <int NA, bool OLD>
__device__ __forceinline__ void pf_stage_commit(const PpoFusedParams& q, int tid, const PfHeadStage<NA>& st, float* sWm, float* sWo, float* sWv) {
    const int A = q.A, H2 = q.H2;
#pragma unroll
    for (int i = 0; i < (PF_H2MAX * NA + 255) / 256; ++i) {
        const int x = tid + 256 * i;
        if (x < H2 * A) { sWm[x] = st.m[i]; if constexpr (OLD) sWo[x] = st.o[i]; }
    }
#pragma unroll
    for (int i = 0; i < PF_NSV; ++i) { const int x = tid + 256 * i; if (x < H2) sWv[x] = st.v[i]; }
}

// the head dot products of a sample's 8 lanes from the rows in registers and the staged kernels: au[a] = h2_pi . Wm[:, a], av = h2_v . Wv, met by the o = 4, 2, 1
// xor shuffles (every lane of the sample ends with the same sums).  MEET = false leaves the shuffles to the caller: the loss body forms the old policy's sums
// behind the dot products and sends them through the same three rounds (with rounds of their own in front of that block the compiler keeps the NA = 2 loss kernels
// at 168 registers instead of 256 + AGPRs, three waves per SIMD instead of one: profiles/r35_ppo_head_helpers.md)
// The staged kernels go in as LDS pointers (callers cast: (pf_lds_cf*)sWm).  As plain pointers they are flat until the address spaces are inferred, and the NA = 8
// kernels then come out with another number of ds_read instructions than the hand-inlined form (same reads executed, other block duplication); typed, every kernel
// keeps its LDS / global instruction counts.  The other helpers take plain pointers: their counts do not move
typedef __attribute__((address_space(3))) const float pf_lds_cf;
typedef __attribute__((address_space(3))) const f32x4 pf_lds_cf4;
template <int NA, int NV, bool MEET = true>
__device__ __forceinline__ void pf_head_sums(pf_lds_cf* sWm, pf_lds_cf* sWv, const f32x4 (&hp)[NV], const f32x4 (&hv)[NV], int part, int nf, int A, float (&au)[NA], float& av) {
    av = 0.f;
#pragma unroll
    for (int a = 0; a < NA; ++a) au[a] = 0.f;
    if constexpr (NA == 2) {                              // exactly two actions (the reference; the host picks this instantiation only then): head-kernel rows of 4 consecutive j are two 16-byte LDS reads
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int f = min(part + 8 * i, nf - 1);      // (threads past the row re-read its last piece: their h2 registers are zero)
            const f32x4 wv = *(pf_lds_cf4*)(sWv + 4 * f);
            const f32x4 wa = *(pf_lds_cf4*)(sWm + 8 * f), wb = *(pf_lds_cf4*)(sWm + 8 * f + 4);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                av += hv[i][e] * wv[e];
                const float w0 = e < 2 ? wa[2 * e] : wb[2 * e - 4], w1 = e < 2 ? wa[2 * e + 1] : wb[2 * e - 3];
                au[0] += hp[i][e] * w0; au[NA > 1 ? 1 : 0] += hp[i][e] * w1;
            }
        }
    } else {
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int f = part + 8 * i;
            if (f >= nf) continue;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int j = 4 * f + e;
                av += hv[i][e] * sWv[j];
                _Pragma("unroll") for (int a = 0; a < NA; ++a) if (a < A) au[a] += hp[i][e] * sWm[j * A + a];
            }
        }
    }
    if constexpr (MEET) {
#pragma unroll
        for (int o = 4; o > 0; o >>= 1) {
            av += __shfl_xor(av, o, 64);
#pragma unroll
            for (int a = 0; a < NA; ++a) au[a] += __shfl_xor(au[a], o, 64);
        }
    }
}

// tanh through the hardware exponential unit (v_exp_f32: ~1 ulp; tanh(u) = 1 - 2 / (e^2u + 1)): the new policy's terms in the loss and clone kernels
__device__ __forceinline__ float pf_fast_tanh(float x) { const float xc = fminf(fmaxf(x, -15.f), 15.f); return 1.0f - 2.0f / (__expf(2.0f * xc) + 1.0f); }

// fixed-order block partial sums: thread k < PF_NPART adds slot k of the block's 32 samples in sample order (behind a barrier)
__device__ __forceinline__ void pf_block_partials(const PpoFusedParams& q, const float (*spart)[PF_NPART], int tid) {
    if (tid < PF_NPART) {
        float sum = 0.f;
        for (int i = 0; i < 32; ++i) sum += spart[i][tid];
        q.partial[(long long)blockIdx.x * PF_NPART + tid] = sum;
    }
}

// head input gradients of this thread's columns of its sample, masked by relu'(h2): from the rows still held in registers.  dh2_pi = relu' sum_a du[a] Wm[j, a],
// dh2_v = relu' dv Wv[j]; VAL = false stores no value-net row
template <int NA, int NV, bool VAL>
__device__ __forceinline__ void pf_head_dh2(const PpoFusedParams& q, const float* sWm, const float* sWv, const float (*sdu)[NA], const float* sdv,
                                            const f32x4 (&hp)[NV], const f32x4 (&hv)[NV], int m, bool mok, int sm, int part) {
    if (!mok) return;
    const int A = q.A, H2 = q.H2, nf = H2 >> 2;
    float* dh2p = q.dh2 + (long long)m * H2; float* dh2v = q.dh2 + (long long)q.M * H2 + (long long)m * H2;
    float dus[NA];
    _Pragma("unroll") for (int a = 0; a < NA; ++a) if (a < A) dus[a] = sdu[sm][a];
    const float dvs = sdv[sm];
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int f = part + 8 * i;
        if (f >= nf) continue;
        f32x4 gp, gv;
        if constexpr (NA == 2) {
            const f32x4 wv = *(const f32x4*)(sWv + 4 * f);
            const f32x4 wa = *(const f32x4*)(sWm + 8 * f), wb = *(const f32x4*)(sWm + 8 * f + 4);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float w0 = e < 2 ? wa[2 * e] : wb[2 * e - 4], w1 = e < 2 ? wa[2 * e + 1] : wb[2 * e - 3];
                float sa = dus[0] * w0;
                sa += dus[NA > 1 ? 1 : 0] * w1;
                gp[e] = hp[i][e] > 0.f ? sa : 0.f;
                gv[e] = hv[i][e] > 0.f ? dvs * wv[e] : 0.f;
            }
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int j = 4 * f + e;
                float sa = 0.f;
                _Pragma("unroll") for (int a = 0; a < NA; ++a) if (a < A) sa += dus[a] * sWm[j * A + a];
                gp[e] = hp[i][e] > 0.f ? sa : 0.f;
                gv[e] = hv[i][e] > 0.f ? dvs * sWv[j] : 0.f;
            }
        }
        *(f32x4*)(dh2p + 4 * f) = gp;
        if constexpr (VAL) *(f32x4*)(dh2v + 4 * f) = gv;
    }
}

// ---- the strided form.  THE BIT-FOR-BIT CONTRACTS.  mi_ppo_logp_old / mi_ppo_old_policy_cache (ppo_predict_head_kernel<NA, 3> with logp_out) fill the caches of
// log pi_old and of the old means.  Three other sites form the same quantities and must give the same bits:
//   the old-policy block of ppo_head_loss_body   the step gives the same parameters whether log pi_old / mu_o come from the cache or from there (in another order
//                                                the two differ by an ulp of log pi_old, and Adam's first step multiplies what that does to a gradient near zero
//                                                by lr / 3.2e-7)
//   ppo_update_stats_head_kernel                 with theta == theta_old its log-probabilities are the cached ones, so d = 0 and r = 1 exactly
//   ppo_kl_stats_head_kernel                     with theta == theta_old its means are the cached ones, so the KL of a policy with itself is 0
// A fourth contract is on the VALUE: ppo_values_head_kernel (mi_ppo_values_idx, the value net run alone) stores for a row what ppo_update_stats_head_kernel's
// value_out stores for it under the same parameters, so a table refreshed by the one can stand where the other's stood.  Both call pf_head_sums_strided<., 8> with
// val = true on the value net's h2 row -- the same columns in the same order, the same three shuffles -- and add bv[0] last; the h2 row is the same bits whichever
// net slot the trunk kernels wrote it to.
// A fifth contract is on the LOG-PROBABILITY of the policy net run alone: ppo_logp_head_kernel (mi_ppo_logp_idx) stores for a row what
// ppo_update_stats_head_kernel's logp_new_out stores for it under the same parameters, and with theta == theta_old what mi_ppo_logp_old cached -- so the V-trace
// weight exp(lp_now - lp_old) of a policy that has not moved is exactly 1.  It calls pf_head_sums_strided<NA, 8> with val = false on net 0's h2 row (the policy
// sums do not depend on val), then pf_mean_libm and pf_logp_term_libm, and sums the terms serially.
// They do because all of them go through the three functions below and sum the actions' terms serially, a = 0, 1, ..: the columns j = part, part + 8, .. of the row
// in ascending order (the loss body spells that loop itself, from LDS: the same values in the same order), the same shuffles, then libm tanhf / expf / logf. ----

// au[a] = sum over this lane's columns j = part, part + TPS, .. of h2p[j] Wm[j, a] (with val: av likewise from h2v and Wv, else 0), then the xor shuffles over the
// sample's TPS lanes.  h2p / h2v: the sample's rows.  val is a constant at two callers and folds through the inlined call; the predict kernel tests it at run time
template <int NA, int TPS>
__device__ __forceinline__ void pf_head_sums_strided(const float* h2p, const float* h2v, const float* Wm, const float* Wv, bool mok, bool val, int part, int H2, int A,
                                                     float (&au)[NA], float& av) {
    av = 0.f;
#pragma unroll
    for (int a = 0; a < NA; ++a) au[a] = 0.f;
    if (mok) {
        for (int j = part; j < H2; j += TPS) {
            const float hp = h2p[j];
            if (val) av += h2v[j] * Wv[j];
            _Pragma("unroll") for (int a = 0; a < NA; ++a) if (a < A) au[a] += hp * Wm[(long long)j * A + a];
        }
    }
#pragma unroll
    for (int o = TPS / 2; o > 0; o >>= 1) {
        av += __shfl_xor(av, o, 64);
#pragma unroll
        for (int a = 0; a < NA; ++a) au[a] += __shfl_xor(au[a], o, 64);
    }
}
// the action mean from the head sum u and the bias b: the tanh squash onto [lo, hi], libm tanhf
__device__ __forceinline__ float pf_mean_libm(float u, float b, float lo, float hi) { return lo + ((tanhf(u + b) + 1.0f) * 0.5f) * (hi - lo); }
// one action's term of log pi(act): libm expf / logf
__device__ __forceinline__ float pf_logp_term_libm(float act, float mean, float logstd) {
    const float sigma = expf(logstd);
    const float z = (act - mean) / sigma;
    return -0.5f * z * z - (PF_HALF_LOG_2PI + logf(sigma));
}

// ordered double-precision reduction of the statistics kernels, no atomics: lanes with part == 0 hold their sample's N terms (the others 0); the 8 samples of a wave
// meet by an xor tree of shuffles (every lane forms the same sums), the four waves' sums in LDS are added in wave order and stored as this block's row of `scratch`
template <int N>
__device__ __forceinline__ void pf_ordered_block_sum(double (&term)[N], double (*swave)[N], double* __restrict__ scratch, int tid) {
#pragma unroll
    for (int k = 0; k < N; ++k) {
#pragma unroll
        for (int o = 8; o < 64; o <<= 1) term[k] += __shfl_xor(term[k], o, 64);
    }
    if ((tid & 63) == 0) {
#pragma unroll
        for (int k = 0; k < N; ++k) swave[tid >> 6][k] = term[k];
    }
    __syncthreads();
    if (tid < N) scratch[(long long)blockIdx.x * N + tid] = ((swave[0][tid] + swave[1][tid]) + swave[2][tid]) + swave[3][tid];
}
// ... and one wave behind it: lane k adds column k of the block rows in block order, then stores (accumulate 0) or adds to (1) stats[k]
template <int N>
__global__ __launch_bounds__(64) void ppo_stats_reduce_kernel(const double* __restrict__ scratch, int n_blocks, int accumulate, double* __restrict__ stats) {
    const int k = threadIdx.x;
    if (k >= N) return;
    double sum = 0.0;
    for (int b = 0; b < n_blocks; ++b) sum += scratch[(long long)b * N + k];
    stats[k] = accumulate ? stats[k] + sum : sum;
}

}  // namespace mi
