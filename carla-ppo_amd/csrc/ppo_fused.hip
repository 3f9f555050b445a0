// ppo_fused.hip — the PPO minibatch step (reference ppo.py:42-66,112-147,218-229) as FIVE launches instead of ~28:
//
//   ppo_l1_kernel         h1 = relu(s W1 + b1)          for the policy, the value net and (unless log pi_old is cached) the old policy
//   ppo_l2_kernel         h2 = relu(h1 W2 + b2)         same nets; the four waves of a block split K = 500
//   ppo_head_loss_kernel  heads (tanh-squashed mean, value), log-probabilities, ratio / clip / value / entropy terms, their gradients
//                         wrt the head pre-activations, per-block loss partial sums, and dh2 = head input gradients masked by relu'(h2)
//   ppo_dh1_kernel        dh1 = (dh2 W2^T) * relu'(h1)
//   ppo_wgrad_kernel      every weight / bias gradient of both nets as independent 32 x 32 tiles, one wave each (dW2 = h1^T dh2, dW1 = s^T dh1,
//                         head kernels, biases as all-ones MFMA rows) and -- single GPU -- its TF-Adam update straight from the accumulators;
//                         one spare wave finalises the loss scalars and logstd
// Behaviour cloning (mi_ppo_clone_step) is the same chain with ppo_head_clone_kernel in the third place -- a supervised loss on the expert's actions -- and, without
// returns, with net 0 alone in every launch (PpoFusedParams::n_wnets).
// The step with a demonstration term (mi_ppo_train_step_demo) is the same chain over M PPO rows + M_demo demonstration rows with ppo_head_demo*_kernel in the third
// place -- the loss body with DEMO = true, which takes the PPO or the clone arithmetic per sample -- and ONE staging launch in front (ppo_demo_stage_kernel gathers
// the state rows of the two tables into [M + M_demo, din]; the layer-1 kernels then read a contiguous minibatch, unchanged).
//
// The head-level kernels are built from the helpers of ppo_head.hpp, each shared piece written once:
//   ppo_head_loss_body (ppo_head_loss[_kl][_vclip]_kernel, ppo_head_demo[_kl][_vclip]_kernel) and ppo_head_clone_kernel:  pf_head_rows, pf_stage_request / pf_stage_commit, pf_head_sums,
//       pf_fast_tanh, pf_block_partials, pf_head_dh2; between them each kernel keeps only its own gathers and its per-sample loss terms.  The loss body's
//       old-policy block also calls pf_mean_libm / pf_logp_term_libm
//   ppo_predict_head_kernel, ppo_update_stats_head_kernel, ppo_kl_stats_head_kernel:  pf_head_sums_strided, pf_mean_libm, pf_logp_term_libm -- the one spelling the
//       bit-for-bit contracts between these kernels and the loss body rest on (stated at those functions); the two statistics kernels end in pf_ordered_block_sum,
//       and ppo_stats_reduce_kernel<N> runs behind either
//   ppo_values_head_kernel (mi_ppo_values_idx: the value net alone, forward only):  pf_head_sums_strided's value half, so that its value is the statistics kernel's
//       value_out bit for bit
// On the host pf_step_head_kernel picks the step's head kernel from a table and pf_na_pick the NA of the other launches; the two rules differ on purpose (A = 1).
//
// All arithmetic is exact fp32 (v_mfma_f32_32x32x2_f32 = fmaf chains; 1e-4 parity with the oracle).  The split-bf16 mode (X3 = true: MI_BF16X3 through
// mi_ppo_set_precision) instantiates the four GEMM kernels with three v_mfma_f32_32x32x16_bf16 per k-block of 16 instead; everything else is shared.  The step is latency bound (78 MFLOP,
// 1.5 MB of weights): what matters is the number of dependent launches and that none of them serialises on one CU.  With FUSE_ADAM the
// gradient never goes through HBM as a separate buffer: the block that finishes a weight tile's gradient (it sums over ALL minibatch rows)
// applies tf.train.AdamOptimizer to that tile at once.  Data parallel (more than one rank) uses the same kernels with FUSE_ADAM = false: they
// write the flat gradient buffer, the host all-reduces it and mi_adam_tf_flat applies the update.
#include <stdio.h>
#include <stdlib.h>
#include "common.hpp"
#include "mi_internal.hpp"
#include "mi355_carla.h"
#include "ppo_fused.hpp"
#include "ppo_head.hpp"

namespace mi {

typedef float f32x16_t __attribute__((ext_vector_type(16)));

__device__ __forceinline__ void pf_mma4(const f32x4& a, const f32x4& b, f32x16_t& c) {
#pragma unroll
    for (int s = 0; s < 4; ++s) c = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s], b[s], c, 0, 0, 0);
}
// D register r of a lane: row 8 (r >> 2) + 4 (lane >> 5) + (r & 3), column lane & 31
__device__ __forceinline__ int pf_row(int r, int lgrp) { return (r & 3) + 8 * (r >> 2) + 4 * lgrp; }

// U k-steps at a time: every operand of the chunk is requested before its first MFMA (a plain loop pays one L2 / HBM latency per step: the
// compiler does not software-pipeline it, and at 32 rows the whole step is nothing but such latencies)
template <int U, class FA, class FB>
__device__ __forceinline__ void pf_mma_chunked(int sb, int se, FA load_a, FB load_b, f32x16_t& acc) {
    for (int s0 = sb; s0 < se; s0 += U) {
        f32x4 a[U], b[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (s0 + u < se) { a[u] = load_a(s0 + u); b[u] = load_b(s0 + u); }
            else { a[u] = f32x4{0.f, 0.f, 0.f, 0.f}; b[u] = f32x4{0.f, 0.f, 0.f, 0.f}; }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) pf_mma4(a[u], b[u], acc);
    }
}

// ---- split-bf16 ("bf16x3") form of the GEMM stages (MI_BF16X3, mi_ppo_set_precision): the operands stay fp32 in HBM and are split in registers by the rule of
// split_from_f32 (common.hpp): hi = RNE-bf16(x), lo = bf16(x - hi).  A k-block of 16 is THREE v_mfma_f32_32x32x16_bf16 -- hi hi, hi lo, lo hi, fp32 accumulation
// (3 x 32 cycles where exact fp32 takes 8 x v_mfma_f32_32x32x2_f32, 8 x 64).  The dropped lo lo term and the halves' own truncation leave ~2^-16 of each
// product.  Operand form of the 32x32x16 MFMA: lane (row r = lane & 31, h = lane >> 5) holds k = 16 s + 8 h + j, j = 0..7, of k-block s.
typedef float f32x8_t __attribute__((ext_vector_type(8)));
__device__ __forceinline__ void pf_split8(const f32x8_t& v, bf16x8& hi, bf16x8& lo) {
    hi = __builtin_convertvector(v, bf16x8);
    lo = __builtin_convertvector(v - __builtin_convertvector(hi, f32x8_t), bf16x8);      // x - hi is exact in fp32
}
__device__ __forceinline__ void pf_mma_x3(const f32x8_t& a, const f32x8_t& b, f32x16_t& c) {
    bf16x8 ah, al, bh, bl;
    pf_split8(a, ah, al);
    pf_split8(b, bh, bl);
    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh, c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl, c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh, c, 0, 0, 0);
}
// column sums of B (the bias rows: all-ones A) kept exact in the split form: three bf16 pieces hold all 24 significand bits of an fp32 value
// (x = hi + mid + lo exactly) and 1.0 times a piece is exact, so only the fp32 accumulation rounds -- as in the exact-fp32 MFMA
__device__ __forceinline__ void pf_colsum_x3(const f32x8_t& b, f32x16_t& c) {
    bf16x8 h, m;
    pf_split8(b, h, m);
    const bf16x8 l = __builtin_convertvector((b - __builtin_convertvector(h, f32x8_t)) - __builtin_convertvector(m, f32x8_t), bf16x8);
    const bf16x8 ones = __builtin_bit_cast(bf16x8, u16x8{0x3F80, 0x3F80, 0x3F80, 0x3F80, 0x3F80, 0x3F80, 0x3F80, 0x3F80});
    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ones, l, c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ones, m, c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ones, h, c, 0, 0, 0);
}
// pf_mma_chunked for k-blocks of 16: U blocks' operands requested before their first MFMA
template <int U, class FA, class FB>
__device__ __forceinline__ void pf_mma_x3_chunked(int sb, int se, FA load_a, FB load_b, f32x16_t& acc) {
    for (int s0 = sb; s0 < se; s0 += U) {
        f32x8_t a[U], b[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (s0 + u < se) { a[u] = load_a(s0 + u); b[u] = load_b(s0 + u); }
            else { a[u] = f32x8_t{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}; b[u] = a[u]; }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) pf_mma_x3(a[u], b[u], acc);
    }
}
__device__ __forceinline__ f32x8_t pf_cat(const f32x4& x, const f32x4& y) { return f32x8_t{x[0], x[1], x[2], x[3], y[0], y[1], y[2], y[3]}; }

// operands through buffer descriptors: rows are clamped, reads past a tensor return 0.0 from the hardware range check, stores past it are dropped --
// no per-lane guard branches (at one wave per SIMD the instruction count is the kernel time: rollout.hip)
#define PF_RSRC(ptr, bytes) __builtin_amdgcn_make_buffer_rsrc((void*)(ptr), 0, (int)(bytes), 0x00020000)
#define PF_OOB 0x40000000u
__device__ __forceinline__ float pf_ld(const __amdgpu_buffer_rsrc_t r, unsigned byte_off) { return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, (int)byte_off, 0, 0)); }
__device__ __forceinline__ f32x4 pf_ld4(const __amdgpu_buffer_rsrc_t r, unsigned byte_off) { return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r, (int)byte_off, 0, 0)); }
__device__ __forceinline__ void pf_st(const __amdgpu_buffer_rsrc_t r, unsigned byte_off, float v) { __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), r, (int)byte_off, 0, 0); }

// TF ApplyAdam on one element
__device__ __forceinline__ void pf_adam(float* p, float* m, float* v, float g, const PpoFusedParams& q) {
    float mm = *m, vv = *v;
    mm += (g - mm) * q.omb1;
    vv += (g * g - vv) * q.omb2;
    *m = mm; *v = vv;
    *p -= (mm * q.alpha) / (sqrtf(vv) + q.epsilon);
}
template <bool FUSE> __device__ __forceinline__ void pf_emit(const PpoFusedParams& q, long long idx, float g, float* gb) {      // gb: q.grads, or this row chunk's slab
    if constexpr (FUSE) pf_adam(q.theta + idx, q.adam_m + idx, q.adam_v + idx, g, q);
    else gb[idx] = g;
}

__device__ __forceinline__ const float* pf_theta(const PpoFusedParams& q, int net) { return net == 2 ? q.theta_old : q.theta; }
// tensor index of (net, which): which 0 W1, 1 b1, 2 W2, 3 b2, 4 head kernel, 5 head bias
__device__ __forceinline__ long long pf_off(const PpoFusedParams& q, int net, int which) { return q.off[(net == 1 ? 7 : 0) + which]; }

// ---------------------------------------------------------------------------------------------------------------------
// layer 1: grid (ceil(H1 / 128), n_nets, ceil(M / 32)); wave w of a block owns the 32-column tile 4 blockIdx.x + w.  K = kin (72): 9 steps (X3: 5 k-blocks).
// ---------------------------------------------------------------------------------------------------------------------
template <bool X3>
__global__ __launch_bounds__(256) void ppo_l1_kernel(const PpoFusedParams q) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lrow = lane & 31, lgrp = lane >> 5;
    const int net = blockIdx.y, m0 = blockIdx.z * 32, n0 = (blockIdx.x * 4 + wave) * 32;
    // the gathered minibatch for the layer-1 filter gradient (rows m0 .. m0 + 31, columns dealt to the 8 half-waves of block column 0) is written BEFORE the
    // tile-range return: with H1 < 128 the waves whose column tile lies past H1 still own their share of the columns (a hidden size of 64 left
    // three quarters of s_gath unwritten)
    if (q.row_idx && q.s_gath && net == 0 && blockIdx.x == 0) {
        const int m = m0 + lrow;
        if (m < q.M) {
            const long long srow_g = min(max(q.row_idx[m], 0), q.n_rows - 1);      // (rows are clamped into the table: a bad index reads a wrong row, never past the buffers)
            for (int k = wave * 2 + lgrp; k < q.din; k += 8) q.s_gath[(long long)m * q.din + k] = q.states[srow_g * q.din + k];
        }
    }
    if (n0 >= q.H1) return;
    const float* th = pf_theta(q, net);
    const float* W = th + pf_off(q, net, 0);
    const float* bias = th + pf_off(q, net, 1);
    const int n = n0 + lrow;
    // states rows are din long, W1 has kin >= din rows of which the last kin - din are zero (and stay zero: their gradient is never formed): a k past
    // din reads the next row's values against a zero weight row -- the load is issued and its value dropped, as in ppo_l1_wide_kernel, so that a NaN in a table
    // row the index does not name stays out (NaN x 0; the demonstration tables of mi_ppo_clone_step); past the tensors the range check returns 0.0
    // (with a row index: the state table has n_rows rows and sample m is its row row_idx[m] -- one dependent load per lane in front of the operand loads)
    const int mrow = min(m0 + lrow, q.M - 1);
    const int srow = q.row_idx ? min(max(q.row_idx[mrow], 0), q.n_rows - 1) : mrow;
    const __amdgpu_buffer_rsrc_t rsS = PF_RSRC(q.states, (long long)(q.row_idx ? q.n_rows : q.M) * q.din * 4), rsW = PF_RSRC(W, (long long)q.kin * q.H1 * 4);
    const unsigned arow = (unsigned)srow * (unsigned)q.din, H1u = (unsigned)q.H1;
    f32x16_t acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    if constexpr (X3) {
        pf_mma_x3_chunked<5>(0, (q.kin + 15) / 16,
            [&](int s_) { const int k = s_ * 16 + lgrp * 8; f32x8_t a;
#pragma unroll
                          for (int e = 0; e < 8; ++e) { const float x = pf_ld(rsS, (arow + (unsigned)(k + e)) * 4u); a[e] = k + e < q.din ? x : 0.f; }
                          return a; },
            [&](int s_) { const unsigned k = (unsigned)(s_ * 16 + lgrp * 8); f32x8_t b;
#pragma unroll
                          for (int e = 0; e < 8; ++e) b[e] = pf_ld(rsW, ((k + e) * H1u + (unsigned)n) * 4u);
                          return b; }, acc);
    } else {
    pf_mma_chunked<9>(0, (q.kin + 7) / 8,
        [&](int s_) { const int k = s_ * 8 + lgrp * 4; f32x4 a;
#pragma unroll
                      for (int e = 0; e < 4; ++e) { const float x = pf_ld(rsS, (arow + (unsigned)(k + e)) * 4u); a[e] = k + e < q.din ? x : 0.f; }
                      return a; },
        [&](int s_) { const unsigned k = (unsigned)(s_ * 8 + lgrp * 4); f32x4 b;
#pragma unroll
                      for (int e = 0; e < 4; ++e) b[e] = pf_ld(rsW, ((k + e) * H1u + (unsigned)n) * 4u);
                      return b; }, acc);
    }
    {
        const float bn = pf_ld(PF_RSRC(bias, (long long)q.H1 * 4), (unsigned)n * 4u);
        const __amdgpu_buffer_rsrc_t rsO = PF_RSRC(q.h1 + (long long)net * q.M * q.H1, (long long)q.M * q.H1 * 4);
        const unsigned col = n < q.H1 ? (unsigned)n * 4u : PF_OOB;
#pragma unroll
        for (int r = 0; r < 16; ++r) pf_st(rsO, (unsigned)(m0 + pf_row(r, lgrp)) * H1u * 4u + col, fmaxf(acc[r] + bn, 0.f));      // rows past M fall outside the descriptor
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// layer 1 at wide K (mi_ppo_set_wide_inputs mode 1, kin > 96): grid (ceil(H1 / 32), n_nets, ceil(M / 32)); the four waves of a block own ONE 32 x 32 output tile and
// split K = kin as ppo_l2_kernel splits H1: wave w takes the contiguous k-steps [w per, min(ksteps, (w + 1) per)), per = ceil(ksteps / 4) (steps of 8; X3: k-blocks
// of 16), requests its share a chunk of 16 steps (X3: 8 k-blocks) at a time -- kin <= 512 is one chunk --, and the partial tiles meet in LDS and are added in that
// kernel's fixed order.  Where ppo_l1_kernel gives one wave the whole K (kin = 520: 65 dependent steps in 8 latency rounds), this is 17 steps in 2.
//   - a wave whose share is empty (X3 at kin = 136: 9 k-blocks, 3 per wave, none for wave 3) runs no step, stores its zero tile and reaches the barrier;
//   - there is no return in front of the barrier: the grid has no column tile past H1;
//   - a k at or past din contributes 0.0 whatever the table holds behind the row (ppo_l1_kernel reads the next row against a zero weight row: NaN x 0 there);
//   - block column 0 of net 0 writes the gathered minibatch s_gath, all of its columns, for every H1.
// ---------------------------------------------------------------------------------------------------------------------
template <bool X3>
__global__ __launch_bounds__(256) void ppo_l1_wide_kernel(const PpoFusedParams q) {
    __shared__ float red[3][16][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lrow = lane & 31, lgrp = lane >> 5;
    const int net = blockIdx.y, m0 = blockIdx.z * 32, n0 = blockIdx.x * 32;
    const int din = q.din;
    if (q.row_idx && q.s_gath && net == 0 && blockIdx.x == 0) {      // rows m0 .. m0 + 31, columns dealt to the block's 8 half-waves
        const int m = m0 + lrow;
        if (m < q.M) {
            const long long srow_g = min(max(q.row_idx[m], 0), q.n_rows - 1);
            for (int k = wave * 2 + lgrp; k < din; k += 8) q.s_gath[(long long)m * din + k] = q.states[srow_g * din + k];
        }
    }
    const float* th = pf_theta(q, net);
    const float* W = th + pf_off(q, net, 0);
    const float* bias = th + pf_off(q, net, 1);
    const int n = n0 + lrow;
    const int ksteps = X3 ? (q.kin + 15) / 16 : (q.kin + 7) / 8, per = (ksteps + 3) / 4;
    const int sb = wave * per, se = min(ksteps, sb + per);
    const int mrow = min(m0 + lrow, q.M - 1);
    const int srow = q.row_idx ? min(max(q.row_idx[mrow], 0), q.n_rows - 1) : mrow;
    // (both sizes are below 2^31 bytes: checked by the host before the launch)
    const __amdgpu_buffer_rsrc_t rsS = PF_RSRC(q.states, (long long)(q.row_idx ? q.n_rows : q.M) * din * 4), rsW = PF_RSRC(W, (long long)q.kin * q.H1 * 4);
    const unsigned arow = (unsigned)srow * (unsigned)din, H1u = (unsigned)q.H1;
    f32x16_t acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    // the state operand: k < din is the row's own entry; a k in [din, kin + 7] is the zero padding -- the load is issued (inside the table or answered 0.0 by the
    // range check) and its value dropped, so that neither a NaN of the next row nor a lane-dependent branch gets in
    if constexpr (X3) {
        pf_mma_x3_chunked<8>(sb, se,
            [&](int s_) { const int k = s_ * 16 + lgrp * 8; f32x8_t a;
#pragma unroll
                          for (int e = 0; e < 8; ++e) { const float x = pf_ld(rsS, (arow + (unsigned)(k + e)) * 4u); a[e] = k + e < din ? x : 0.f; }
                          return a; },
            [&](int s_) { const unsigned k = (unsigned)(s_ * 16 + lgrp * 8); f32x8_t b;
#pragma unroll
                          for (int e = 0; e < 8; ++e) b[e] = pf_ld(rsW, ((k + e) * H1u + (unsigned)n) * 4u);
                          return b; }, acc);
    } else {
        pf_mma_chunked<16>(sb, se,
            [&](int s_) { const int k = s_ * 8 + lgrp * 4; f32x4 a;
#pragma unroll
                          for (int e = 0; e < 4; ++e) { const float x = pf_ld(rsS, (arow + (unsigned)(k + e)) * 4u); a[e] = k + e < din ? x : 0.f; }
                          return a; },
            [&](int s_) { const unsigned k = (unsigned)(s_ * 8 + lgrp * 4); f32x4 b;
#pragma unroll
                          for (int e = 0; e < 4; ++e) b[e] = pf_ld(rsW, ((k + e) * H1u + (unsigned)n) * 4u);
                          return b; }, acc);
    }
    if (wave > 0) {
#pragma unroll
        for (int r = 0; r < 16; ++r) red[wave - 1][r][lane] = acc[r];
    }
    __syncthreads();
    if (wave == 0) {
        const float bn = pf_ld(PF_RSRC(bias, (long long)q.H1 * 4), (unsigned)n * 4u);
        const __amdgpu_buffer_rsrc_t rsO = PF_RSRC(q.h1 + (long long)net * q.M * q.H1, (long long)q.M * q.H1 * 4);
        const unsigned col = n < q.H1 ? (unsigned)n * 4u : PF_OOB;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float v = ((acc[r] + red[0][r][lane]) + (red[1][r][lane] + red[2][r][lane]));
            pf_st(rsO, (unsigned)(m0 + pf_row(r, lgrp)) * H1u * 4u + col, fmaxf(v + bn, 0.f));      // rows past M fall outside the descriptor
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// layer 2: grid (ceil(H2 / 32), n_nets, ceil(M / 32)); the four waves split K = H1, partial tiles meet in LDS.
// ---------------------------------------------------------------------------------------------------------------------
template <bool X3>
__global__ __launch_bounds__(256) void ppo_l2_kernel(const PpoFusedParams q) {
    __shared__ float red[3][16][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lrow = lane & 31, lgrp = lane >> 5;
    const int net = blockIdx.y, m0 = blockIdx.z * 32, n0 = blockIdx.x * 32;
    const float* th = pf_theta(q, net);
    const float* W = th + pf_off(q, net, 2);
    const float* bias = th + pf_off(q, net, 3);
    const float* x = q.h1 + (long long)net * q.M * q.H1;
    const int K = q.H1;
    const int ksteps = X3 ? (K + 15) / 16 : (K + 7) / 8, per = (ksteps + 3) / 4;
    const int sb = wave * per, se = min(ksteps, sb + per);
    const int n = n0 + lrow;
    const __amdgpu_buffer_rsrc_t rsX = PF_RSRC(x, (long long)q.M * K * 4), rsW = PF_RSRC(W, (long long)K * q.H2 * 4);
    const unsigned arow = (unsigned)min(m0 + lrow, q.M - 1) * (unsigned)K, H2u = (unsigned)q.H2;
    f32x16_t acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    if constexpr (X3) {
        pf_mma_x3_chunked<8>(sb, se,
            [&](int s_) { const unsigned k = arow + (unsigned)(s_ * 16 + lgrp * 8); return pf_cat(pf_ld4(rsX, k * 4u), pf_ld4(rsX, (k + 4u) * 4u)); },
            [&](int s_) { const unsigned k = (unsigned)(s_ * 16 + lgrp * 8); f32x8_t b;
#pragma unroll
                          for (int e = 0; e < 8; ++e) b[e] = pf_ld(rsW, ((k + e) * H2u + (unsigned)n) * 4u);
                          return b; }, acc);
    } else {
    pf_mma_chunked<16>(sb, se,                            // K % 4 == 0; a k past K reads the next row of x against weights past the tensor (0.0)
        [&](int s_) { return pf_ld4(rsX, (arow + (unsigned)(s_ * 8 + lgrp * 4)) * 4u); },
        [&](int s_) { const unsigned k = (unsigned)(s_ * 8 + lgrp * 4); f32x4 b;
#pragma unroll
                      for (int e = 0; e < 4; ++e) b[e] = pf_ld(rsW, ((k + e) * H2u + (unsigned)n) * 4u);
                      return b; }, acc);
    }
    if (wave > 0) {
#pragma unroll
        for (int r = 0; r < 16; ++r) red[wave - 1][r][lane] = acc[r];
    }
    __syncthreads();
    if (wave == 0) {
        const float bn = pf_ld(PF_RSRC(bias, (long long)q.H2 * 4), (unsigned)n * 4u);
        const __amdgpu_buffer_rsrc_t rsO = PF_RSRC(q.h2 + (long long)net * q.M * q.H2, (long long)q.M * q.H2 * 4);
        const unsigned col = n < q.H2 ? (unsigned)n * 4u : PF_OOB;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float v = ((acc[r] + red[0][r][lane]) + (red[1][r][lane] + red[2][r][lane]));
            pf_st(rsO, (unsigned)(m0 + pf_row(r, lgrp)) * H2u * 4u + col, fmaxf(v + bn, 0.f));
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// heads + loss + head input gradients: grid ceil(M / 32) blocks of 256 threads; a block owns 32 samples, 8 threads per sample.
//   u[m,a] = h2_pi[m,:] Wm[:,a] + bm[a] (same for the old policy), vraw[m] = h2_v[m,:] Wv + bv
//   mean = low + (tanh(u)+1)/2 (high-low) ; logp = sum_a -.5 z^2 - (.5 log 2pi + log sigma) ; ratio = exp(logp - logp_old)
//   loss = -mean(min(r A, clip(r) A)) + vs mean((V-R)^2) - es sum_a(entropy)        (ppo.py:58-66,112-132; tf.minimum's tie rule)
//   du, dv = d loss / d head pre-activations ; dh2_pi[m,j] = relu'(h2) sum_a du[m,a] Wm[j,a] ; dh2_v[m,j] = relu'(h2) dv[m] Wv[j]
// Every thread requests its whole share of the policy's and the value net's h2 rows (<= 10 float4 each) before anything is used, the head kernels are staged in
// LDS meanwhile, and the same registers produce dh2 at the end: one memory latency for the whole kernel.  (Without a cached log pi_old the old policy's h2 row is
// requested with them, in the column order of the kernel that fills that cache, see below.)
//
// VCLIP (ppo_head_loss_vclip_kernel; mi_ppo_train_step_vclip): the clipped value loss of the original PPO2 code (baselines ppo2, tf.clip_by_value + tf.maximum).
// Per sample, with V the value head's output under theta, V_old = q.v_old[row] the value recorded when the data was collected, R the return, eps_v = q.clip_range_vf > 0:
//   V_c  = min(max(V, V_old - eps_v), V_old + eps_v)     a clamp of V itself, so V_c == V bit for bit inside the range
//   l_u  = (V - R)^2 ,  l_c = (V_c - R)^2
//   value_loss = value_scale * mean(max(l_u, l_c))        the max form of baselines ppo2, not the V_c-only form
//   dLoss/dV   = (l_c > l_u) ? 0 : 2 * value_scale * (V - R) / M_global
// tf.maximum's tie rule: on a tie the gradient goes to the first argument.  Inside the range and at its edge both terms are the same number, so the plain gradient
// flows; the clipped branch is chosen only outside the range, where its slope is 0.  eps_v = +inf gives the unclipped step bit for bit.  V_old is one more 4-byte
// gather per sample, requested with returns / advantages / log pi_old (the same clamped table row) before the first barrier; nothing on the policy side changes, and
// the partial layout, the LDS and the finalisation in ppo_wgrad_kernel are those of the plain kernel.
//
// KLP (ppo_head_loss_kl[_vclip]_kernel; mi_ppo_train_step_kl): the KL-penalised surrogate of the PPO paper (Schulman et al. 2017, section 4) on top of the clip.
// Direction KL(pi_old || pi_theta), closed form for the diagonal Gaussian.  Per (sample m, action a), with ls / lso the current / old action_logstd, mu / mu_o the
// current / old action means (after the low + (tanh(u) + 1) / 2 (high - low) map), d = ls - lso, D = mu - mu_o, sigma = exp(ls), beta = q.kl_coef >= 0:
//   KL[m,a] = d + expm1(-2 d) / 2 + D^2 / (2 sigma^2) ,  KL[m] = sum_a KL[m,a] ,  loss += beta mean_m KL[m]
//   du[m,a]    += beta inv_m (D / sigma^2) (high - low) / 2 (1 - t^2)
//   dlogstd[a] += beta inv_m sum_m (-expm1(-2 d) - D^2 / sigma^2)          (summed per sample with inv_m = 1 / M_global: no grad_scale, unlike the entropy term)
// Lane `part` of a sample forms the terms of action `part` from mean, t, sigma it already holds; the per-sample KL meets with lp_n's shuffles; the du / dlogstd
// terms are added into sdu / du / spart[3 + part], so nothing behind this kernel changes.  mu_o: with a cached log pi_old one more 4-byte gather per (sample,
// action) from q.mean_old at the clamped row mr, requested with actions / returns / advantage; without a cache it is the mean the old-policy block below forms
// (tanhf, the cache kernel's spelling: both sources give the same mu_o).  lso comes from theta_old in both.  The block's sum of KL[m] (samples in order, one
// thread) goes to q.kl_partial[block]; ppo_wgrad_kernel's spare wave adds those in block order.  beta = 0 measures: every added term is 0.
// ---------------------------------------------------------------------------------------------------------------------
//
// DUAL CLIP (mi_ppo_set_dual_clip; every instantiation, a run-time value): q.dual_clip = c > 1, or +inf with the setting off.  Behind s = min(s1, s2) a PPO row with
// A < 0 and c A > s takes the constant c A: its policy partial is c A and dr = 0, so the surrogate adds exactly 0.0 to du and to dlogstd; the KL penalty's own terms,
// the value side and demonstration rows are as they were.  One multiply, two compares, two selects per lane; with c = +inf no comparison holds and every stored
// bit is the plain step's (profiles/r42_dual_clip.md: why this is a field of PpoFusedParams and not a template flag).
//
// DEMO (ppo_head_demo[_kl][_vclip]_kernel; mi_ppo_train_step_demo): the step over M = m_ppo + M_demo rows of which rows m >= q.m_ppo are DEMONSTRATION rows.  A
// demonstration row takes the arithmetic of ppo_head_clone_kernel (policy only), operation for operation, with inv_m_demo in the place of inv_m, and then the
// weight c_d = q.demo_coef on du and on the logstd term: it gathers its expert action from q.demo_actions at row demo_row_idx[m - m_ppo] (clamped; nullptr:
// row m - m_ppo), reads no return, advantage, old policy or value target, leaves dv = 0.0 exactly, slots 0 - 2 and the action-mean slots of the block partials 0
// (the PPO scalars are over PPO rows), KL[m] = 0, and its l[m] and squared error in sdemo -> q.demo_partial[block][2], added in block order by ppo_wgrad_kernel's
// spare wave.  The 8 lanes of a sample take one path; the one wave that holds row m_ppo diverges.  With DEMO = false nothing of this is compiled: the eight
// kernels of the other entries are the code they were.
template <int NA, bool VCLIP, bool KLP, bool DEMO = false>
__device__ __forceinline__ void ppo_head_loss_body(const PpoFusedParams& q) {
    __shared__ __attribute__((aligned(16))) float sWm[PF_H2MAX * PF_MAX_ACT], sWo[PF_H2MAX * PF_MAX_ACT], sWv[PF_H2MAX];
    __shared__ float su[32][NA], sv[32], sdu[32][NA], sdv[32], spart[32][PF_NPART];
    __shared__ float skl[KLP ? 32 : 1];                   // KLP: KL[m] of the block's samples
    __shared__ float sdemo[DEMO ? 32 : 1][2];             // DEMO: l[m] and the squared error of the block's demonstration rows (0 at PPO rows)
    const int tid = threadIdx.x, m0 = blockIdx.x * 32, A = q.A, H2 = q.H2;
    const float* __restrict__ bm = q.theta + q.off[5]; const float* __restrict__ bmo = q.theta_old + q.off[5]; const float* __restrict__ bv = q.theta + q.off[12];
    const float* __restrict__ h2o = q.h2 + 2ll * q.M * H2;
    const bool old_net = q.logp_old == nullptr;
    const int sm = tid >> 3, part = tid & 7, m = m0 + sm;
    const bool mok = m < q.M;
    const bool demo = DEMO && mok && m >= q.m_ppo;        // a demonstration row (all 8 lanes of the sample agree)
    f32x4 hp[PF_NV], hv[PF_NV];
    pf_head_rows<PF_NV, true>(q, m, mok, part, hp, hv);
    // the old policy's row (only without a cached log pi_old), requested with the others: this thread's columns are j = part, part + 8, .. as in the kernel that
    // fills the cache (see the head sums below), so single floats instead of 16-byte pieces
    constexpr int NH = PF_H2MAX / 8;                      // columns per thread (40)
    float ho[NH];
    if (old_net) {                                        // (uniform: with a cache none of this is issued)
#pragma unroll
        for (int k = 0; k < NH; ++k) { const int j = part + 8 * k; ho[k] = (mok && j < H2) ? h2o[(long long)m * H2 + j] : 0.f; }
    } else {
#pragma unroll
        for (int k = 0; k < NH; ++k) ho[k] = 0.f;
    }
    // head kernels -> LDS through registers (all requests in flight together), and the per-sample scalars the loss thread will need
    PfHeadStage<NA> st;
    pf_stage_request<NA, true, true>(q, tid, old_net, st);
    float p_act[NA], p_adv_s = 0.f, p_ret_s = 0.f, p_lpo_s = 0.f, p_vold_s = 0.f, p_muo_s = 0.f, p_ls[NA], p_lso[NA], p_lo[NA], p_hi[NA];
    int mr = (q.row_idx && mok) ? min(max(q.row_idx[m], 0), q.n_rows - 1) : m;     // the sample's row in the horizon-batch tables (actions / returns / advantages / cached log pi_old)
    const float* __restrict__ acts = q.actions;
    if constexpr (DEMO) {                                 // ... or in the demonstration tables
        if (demo) { mr = q.demo_row_idx ? min(max(q.demo_row_idx[m - q.m_ppo], 0), q.n_demo_rows - 1) : m - q.m_ppo; acts = q.demo_actions; }
    }
#pragma unroll
    for (int a = 0; a < NA; ++a) {
        const bool aok = a < A;
        p_act[a] = (mok && aok) ? acts[(long long)mr * A + a] : 0.f;
        p_ls[a] = aok ? q.theta[q.off[6] + a] : 0.f; p_lso[a] = (aok && (old_net || KLP)) ? q.theta_old[q.off[6] + a] : 0.f;
        p_lo[a] = aok ? q.low[a] : 0.f; p_hi[a] = aok ? q.high[a] : 0.f;
    }
    if (mok && !demo) { p_adv_s = q.adv[mr]; p_ret_s = q.returns[mr]; if (!old_net) p_lpo_s = q.logp_old[mr]; }
    if constexpr (VCLIP) { if (mok && !demo) p_vold_s = q.v_old[mr]; }
    if constexpr (KLP) { if (mok && !demo && !old_net && part < A) p_muo_s = q.mean_old[(long long)mr * A + part]; }
    pf_stage_commit<NA, true>(q, tid, st, sWm, sWo, sWv);
    __syncthreads();
    float lp_old_s = 0.f;
    {
        float au[NA], ao[NA], av;
#pragma unroll
        for (int a = 0; a < NA; ++a) ao[a] = 0.f;
        pf_head_sums<NA, PF_NV, false>((pf_lds_cf*)sWm, (pf_lds_cf*)sWv, hp, hv, part, H2 >> 2, A, au, av);
        // the old policy's log pi_old and means, in the strided form that fills the caches of them (the contracts: ppo_head.hpp): columns j = part, part + 8, ..
        // of the row in ascending order against the old head kernel (here from LDS: the same values), pf_head_sums_strided's shuffles, then the libm spellings
        // and a serial sum over the actions.  The price is paid only without a cache: up to A libm chains per thread where the new policy's terms go through
        // the hardware units (see below)
        if (old_net && mok) {
#pragma unroll
            for (int k = 0; k < NH; ++k) {
                const int j = part + 8 * k;
                if (j >= H2) continue;
                _Pragma("unroll") for (int a = 0; a < NA; ++a) if (a < A) ao[a] += ho[k] * sWo[j * A + a];
            }
        }
#pragma unroll
        for (int o = 4; o > 0; o >>= 1) {                 // (pf_head_sums' rounds, MEET = false, with ao in them: see there)
            av += __shfl_xor(av, o, 64);
#pragma unroll
            for (int a = 0; a < NA; ++a) { au[a] += __shfl_xor(au[a], o, 64); ao[a] += __shfl_xor(ao[a], o, 64); }
        }
        if (old_net) {                                    // (all 8 threads of a sample hold the same sums and form the same value)
            float lp = 0.f;
            _Pragma("unroll") for (int a = 0; a < NA; ++a) if (a < A) {
                const float mean = pf_mean_libm(ao[a], bmo[a], p_lo[a], p_hi[a]);
                lp += pf_logp_term_libm(p_act[a], mean, p_lso[a]);
                if constexpr (KLP) { if (a == part) p_muo_s = mean; }
            }
            lp_old_s = lp;
        }
        if (part == 0) {
            sv[sm] = av + bv[0];
            _Pragma("unroll") for (int a = 0; a < NA; ++a) if (a < A) su[sm][a] = au[a] + bm[a];
        }
    }
    __syncthreads();
    // ---- per-sample loss terms: lane `part` of a sample's 8 threads owns action `part` of the new policy, the terms meet by shuffles (log pi_old: lp_old_s above, or the cache).
    //      exp / log / tanh through the hardware transcendental units (v_exp_f32 / v_log_f32: ~1 ulp; tanh(u) = 1 - 2 / (e^2u + 1)): the
    //      libm sequences are ~100-instruction dependent chains, which at one wave per block was most of this kernel ----
    if (DEMO && demo) {
        // a demonstration row: ppo_head_clone_kernel's terms (policy only), then the weight c_d
        float act = 0.f, ls = 0.f, lo = 0.f, hi = 0.f;
#pragma unroll
        for (int a = 0; a < NA; ++a) if (a == part) { act = p_act[a]; ls = p_ls[a]; lo = p_lo[a]; hi = p_hi[a]; }
        float l = 0.f, sq = 0.f, d = 0.f, dls = 0.f, mean = 0.f;
        const bool aok = part < A;
        if (aok) {
            const float t = pf_fast_tanh(su[sm][part < NA ? part : 0]);
            mean = lo + ((t + 1.0f) * 0.5f) * (hi - lo);
            const float diff = mean - act, sl = (0.5f * (hi - lo)) * (1.0f - t * t);
            sq = diff * diff;
            if (q.demo_kind == 1) {
                l = sq;
                d = (2.0f * diff) * sl * q.inv_m_demo;
            } else {
                const float sigma = __expf(ls);
                const float z = (act - mean) / sigma;
                l = 0.5f * z * z + (ls + PF_HALF_LOG_2PI);
                d = -((z / sigma) * sl) * q.inv_m_demo;
                dls = (1.0f - z * z) * q.inv_m_demo;
            }
            d *= q.demo_coef; dls *= q.demo_coef;
            if (q.mean_out) q.mean_out[(long long)m * A + part] = mean;
        }
#pragma unroll
        for (int o = 4; o > 0; o >>= 1) { l += __shfl_xor(l, o, 64); sq += __shfl_xor(sq, o, 64); }
        if (part < NA) sdu[sm][part < NA ? part : 0] = aok ? d : 0.f;
        if (aok) q.du[(long long)m * A + part] = d;
#pragma unroll
        for (int k = part; k < PF_NPART; k += 8) spart[sm][k] = 0.f;
        __builtin_amdgcn_wave_barrier();
        if (part == 0) {
            sdv[sm] = 0.f; q.dv[m] = 0.f;
            if constexpr (KLP) skl[sm] = 0.f;
            if (q.logp_out) q.logp_out[m] = 0.f;
            sdemo[sm][0] = l; sdemo[sm][1] = sq;
        }
        if (aok) spart[sm][3 + part] = dls;
    } else {
        float lp_n = 0.f, dl = 0.f, zsq = 0.f, mean = 0.f;
        float act = 0.f, ls = 0.f, lo = 0.f, hi = 0.f;
        float lso = 0.f, kl = 0.f, kdu = 0.f, kdls = 0.f;  // KLP: this lane's old logstd, KL[m,part] and the penalty's du / dlogstd terms (without beta inv_m)
#pragma unroll
        for (int a = 0; a < NA; ++a) if (a == part) { act = p_act[a]; ls = p_ls[a]; lo = p_lo[a]; hi = p_hi[a]; if constexpr (KLP) lso = p_lso[a]; }
        const bool aok = part < A && mok;
        if (aok) {
            const float t = pf_fast_tanh(su[sm][part < NA ? part : 0]);
            mean = lo + ((t + 1.0f) * 0.5f) * (hi - lo);
            const float sigma = __expf(ls);
            const float z = (act - mean) / sigma;
            lp_n = -0.5f * z * z - (PF_HALF_LOG_2PI + __logf(sigma));
            dl = (z / sigma) * (0.5f * (hi - lo)) * (1.0f - t * t);
            zsq = z * z;
            if (q.mean_out) q.mean_out[(long long)m * A + part] = mean;
            if constexpr (KLP) {
                const float dd = ls - lso, dm = mean - p_muo_s, em = expm1f(-2.0f * dd);
                const float qv = (dm * dm) / (sigma * sigma);          // D^2 / sigma^2
                kl = dd + 0.5f * em + 0.5f * qv;
                kdu = (dm / (sigma * sigma)) * (0.5f * (hi - lo)) * (1.0f - t * t);
                kdls = -em - qv;
            }
        }
#pragma unroll
        for (int o = 4; o > 0; o >>= 1) lp_n += __shfl_xor(lp_n, o, 64);
        if constexpr (KLP) {
#pragma unroll
            for (int o = 4; o > 0; o >>= 1) kl += __shfl_xor(kl, o, 64);
        }
        const float lp_o = old_net ? lp_old_s : p_lpo_s;
        const float r = __expf(lp_n - lp_o);
        const float ad = p_adv_s;
        const float rc = fminf(fmaxf(r, 1.0f - q.clip_eps), 1.0f + q.clip_eps);
        const float s1 = r * ad, s2 = rc * ad;
        // dual clip (mi_ppo_set_dual_clip; q.dual_clip = c > 1, +inf with the setting off): a sample with A < 0 whose c A lies above min(s1, s2) takes c A, a
        // constant of theta, so dr = 0 as on the clipped branch.  tf.maximum's tie rule: on a tie s keeps the gradient.  A >= 0 (-0.0 included) never takes it;
        // with c = +inf c A is -inf (NaN at A = 0, where A < 0 fails first) and no comparison holds: every stored bit is the plain step's
        const float sm12 = fminf(s1, s2), ca = q.dual_clip * ad;
        const bool dual = ad < 0.f && ca > sm12;
        const float dr = (s1 <= s2 && !dual) ? ad : 0.f;  // tf.minimum: gradient to the first argument on ties; the clipped branches have zero slope
        const float coef = -dr * r * q.inv_m;
        float d = coef * dl;
        const float kb = KLP ? q.kl_coef * q.inv_m : 0.f;
        if constexpr (KLP) d += kb * kdu;
        if (part < NA) sdu[sm][part < NA ? part : 0] = aok ? d : 0.f;
        if (aok) q.du[(long long)m * A + part] = d;
        const float dvv = sv[sm] - p_ret_s;
        float dvm = mok ? 2.0f * q.value_scale * dvv * q.inv_m : 0.f;
        float lv = dvv * dvv;
        if constexpr (VCLIP) {                            // (see the header: the clamp of V itself, tf.maximum's tie rule)
            const float vcl = fminf(fmaxf(sv[sm], p_vold_s - q.clip_range_vf), p_vold_s + q.clip_range_vf);
            const float dvc = vcl - p_ret_s;
            const float l_c = dvc * dvc;
            if (l_c > lv) dvm = 0.f;
            lv = fmaxf(lv, l_c);
        }
#pragma unroll
        for (int k = part; k < PF_NPART; k += 8) spart[sm][k] = 0.f;
        __builtin_amdgcn_wave_barrier();
        if (part == 0) {
            sdv[sm] = dvm;
            if constexpr (KLP) skl[sm] = mok ? kl : 0.f;
            if constexpr (DEMO) { sdemo[sm][0] = 0.f; sdemo[sm][1] = 0.f; }
            if (mok) { q.dv[m] = dvm; if (q.logp_out) q.logp_out[m] = lp_n; spart[sm][0] = dual ? ca : sm12; spart[sm][1] = lv; spart[sm][2] = r; }
        }
        if (aok) {
            float dls = coef * (zsq - 1.0f);
            if constexpr (KLP) dls += kb * kdls;
            spart[sm][3 + part] = dls; spart[sm][3 + PF_MAX_ACT + part] = mean;
        }
    }
    __syncthreads();
    pf_block_partials(q, spart, tid);
    if constexpr (KLP) {
        if (tid == 32) {                                  // the block's KL sum, samples in order
            float sum = 0.f;
            for (int i = 0; i < 32; ++i) sum += skl[i];
            q.kl_partial[blockIdx.x] = sum;
        }
    }
    if constexpr (DEMO) {
        if (tid == 33 || tid == 34) {                     // the block's demonstration sums, samples in order
            float sum = 0.f;
            for (int i = 0; i < 32; ++i) sum += sdemo[i][tid - 33];
            q.demo_partial[(long long)blockIdx.x * 2 + (tid - 33)] = sum;
        }
    }
    pf_head_dh2<NA, PF_NV, true>(q, sWm, sWv, sdu, sdv, hp, hv, m, mok, sm, part);
}
template <int NA> __global__ __launch_bounds__(256) void ppo_head_loss_kernel(const PpoFusedParams q) { ppo_head_loss_body<NA, false, false>(q); }
template <int NA> __global__ __launch_bounds__(256) void ppo_head_loss_vclip_kernel(const PpoFusedParams q) { ppo_head_loss_body<NA, true, false>(q); }
template <int NA> __global__ __launch_bounds__(256) void ppo_head_loss_kl_kernel(const PpoFusedParams q) { ppo_head_loss_body<NA, false, true>(q); }
template <int NA> __global__ __launch_bounds__(256) void ppo_head_loss_kl_vclip_kernel(const PpoFusedParams q) { ppo_head_loss_body<NA, true, true>(q); }
template <int NA> __global__ __launch_bounds__(256) void ppo_head_demo_kernel(const PpoFusedParams q) { ppo_head_loss_body<NA, false, false, true>(q); }
template <int NA> __global__ __launch_bounds__(256) void ppo_head_demo_vclip_kernel(const PpoFusedParams q) { ppo_head_loss_body<NA, true, false, true>(q); }
template <int NA> __global__ __launch_bounds__(256) void ppo_head_demo_kl_kernel(const PpoFusedParams q) { ppo_head_loss_body<NA, false, true, true>(q); }
template <int NA> __global__ __launch_bounds__(256) void ppo_head_demo_kl_vclip_kernel(const PpoFusedParams q) { ppo_head_loss_body<NA, true, true, true>(q); }

// the rows the demonstration step's chain reads: out [M, din], row m < m_ppo = PPO state row row_idx[m] (clamped; nullptr: m), row m >= m_ppo = demonstration
// state row demo_row_idx[m - m_ppo] (likewise).  One thread per element, 64-bit offsets into the tables; a row no index names is never read
__global__ __launch_bounds__(256) void ppo_demo_stage_kernel(const float* __restrict__ states, const int* __restrict__ row_idx, int n_rows, int m_ppo,
                                                             const float* __restrict__ demo_states, const int* __restrict__ demo_row_idx, int n_demo_rows, int M, int din,
                                                             float* __restrict__ out) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)M * din) return;
    const int m = (int)(i / din), k = (int)(i - (long long)m * din);
    float v;
    if (m < m_ppo) { const long long r = row_idx ? min(max(row_idx[m], 0), n_rows - 1) : m; v = states[r * din + k]; }
    else { const int md = m - m_ppo; const long long r = demo_row_idx ? min(max(demo_row_idx[md], 0), n_demo_rows - 1) : md; v = demo_states[r * din + k]; }
    out[i] = v;
}

// ---------------------------------------------------------------------------------------------------------------------
// CLONE (ppo_head_clone_kernel; mi_ppo_clone_step): behaviour cloning, the supervised form of the head / loss kernel.  A kernel of its own, built from the same
// helpers (ppo_head.hpp): it keeps no sWo and no old-policy row, and the eight instantiations above stay as they are.  q.actions holds the EXPERT's actions a_E (a table with row_idx), q.clone the kind + 1, q.returns the returns or nullptr.
// Per sample m and action a, with t = tanh(u), mean = lo + (t + 1) / 2 (hi - lo), sigma = exp(logstd[a]), z = (a_E - mean) / sigma:
//   kind 0 "nll":  l[m] = sum_a (z^2 / 2 + logstd[a] + log(2 pi) / 2) ;  dl/du = -(z / sigma) (hi - lo) / 2 (1 - t^2) ;  dl/dlogstd[a] = 1 - z^2
//   kind 1 "mse":  l[m] = sum_a (mean - a_E)^2 ;  dl/du = 2 (mean - a_E) (hi - lo) / 2 (1 - t^2) ;  dl/dlogstd = 0 exactly
//   value term (only with returns): value_scale (V - R)^2 ,  dV = 2 value_scale (V - R) inv_m          -- the arithmetic of ppo_head_loss_body, operation for operation
//   clone_loss = inv_m sum_m l[m] ,  loss = clone_loss + value_loss
// No old policy, no advantage, no ratio, no clip, no entropy term (the call's entropy_scale is 0: ppo_wgrad_kernel's spare wave adds nothing to the logstd
// gradient).  Partial slots: 0 l[m], 1 (V - R)^2, 2 sum_a (mean - a_E)^2 in BOTH kinds (mean_sq_error), 3 + a dl/dlogstd[a] inv_m, 3 + PF_MAX_ACT + a mean.
// Without returns (policy only) nothing of the value net is read or written: no h2 row of net 1, no value head, no dv, no dh2 of net 1; slot 1 is 0.
// As above: 8 lanes per sample, lane `part` owns action `part`, hardware transcendentals, fixed-order block sums, du / dv / dh2 for the chain behind.
// ---------------------------------------------------------------------------------------------------------------------
// VAL (returns given) is a template flag, not a test of q.returns: see pf_head_rows.
template <int NA, bool VAL>
__global__ __launch_bounds__(256) void ppo_head_clone_kernel(const PpoFusedParams q) {
    __shared__ __attribute__((aligned(16))) float sWm[PF_H2MAX * PF_MAX_ACT], sWv[PF_H2MAX];
    __shared__ float su[32][NA], sv[32], sdu[32][NA], sdv[32], spart[32][PF_NPART];
    const int tid = threadIdx.x, m0 = blockIdx.x * 32, A = q.A, H2 = q.H2;
    const bool mse = q.clone == 2;
    const float* __restrict__ bm = q.theta + q.off[5]; const float* __restrict__ bv = q.theta + q.off[12];
    const int sm = tid >> 3, part = tid & 7, m = m0 + sm;
    const bool mok = m < q.M;
    f32x4 hp[PF_NV], hv[PF_NV];
    pf_head_rows<PF_NV, VAL>(q, m, mok, part, hp, hv);
    PfHeadStage<NA> st;
    pf_stage_request<NA, false, VAL>(q, tid, false, st);
    const int mr = (q.row_idx && mok) ? min(max(q.row_idx[m], 0), q.n_rows - 1) : m;     // the sample's row in the tables (expert actions / returns)
    float act = 0.f, ls = 0.f, lo = 0.f, hi = 0.f, p_ret_s = 0.f;                        // lane `part`: its action's scalars
    if (part < A) { ls = q.theta[q.off[6] + part]; lo = q.low[part]; hi = q.high[part]; if (mok) act = q.actions[(long long)mr * A + part]; }
    if (VAL && mok) p_ret_s = q.returns[mr];
    pf_stage_commit<NA, false>(q, tid, st, sWm, nullptr, sWv);
    __syncthreads();
    {
        float au[NA], av;
        pf_head_sums<NA, PF_NV>((pf_lds_cf*)sWm, (pf_lds_cf*)sWv, hp, hv, part, H2 >> 2, A, au, av);
        if (part == 0) {
            sv[sm] = VAL ? av + bv[0] : 0.f;
            _Pragma("unroll") for (int a = 0; a < NA; ++a) if (a < A) su[sm][a] = au[a] + bm[a];
        }
    }
    __syncthreads();
    {
        float l = 0.f, sq = 0.f, d = 0.f, dls = 0.f, mean = 0.f;
        const bool aok = part < A && mok;
        if (aok) {
            const float t = pf_fast_tanh(su[sm][part < NA ? part : 0]);
            mean = lo + ((t + 1.0f) * 0.5f) * (hi - lo);
            const float diff = mean - act, sl = (0.5f * (hi - lo)) * (1.0f - t * t);
            sq = diff * diff;
            if (mse) {
                l = sq;
                d = (2.0f * diff) * sl * q.inv_m;
            } else {
                const float sigma = __expf(ls);
                const float z = (act - mean) / sigma;
                l = 0.5f * z * z + (ls + PF_HALF_LOG_2PI);
                d = -((z / sigma) * sl) * q.inv_m;
                dls = (1.0f - z * z) * q.inv_m;
            }
            if (q.mean_out) q.mean_out[(long long)m * A + part] = mean;
        }
#pragma unroll
        for (int o = 4; o > 0; o >>= 1) { l += __shfl_xor(l, o, 64); sq += __shfl_xor(sq, o, 64); }
        if (part < NA) sdu[sm][part < NA ? part : 0] = aok ? d : 0.f;
        if (aok) q.du[(long long)m * A + part] = d;
        const float dvv = sv[sm] - p_ret_s;
        const float dvm = (mok && VAL) ? 2.0f * q.value_scale * dvv * q.inv_m : 0.f;
        const float lv = dvv * dvv;
#pragma unroll
        for (int k = part; k < PF_NPART; k += 8) spart[sm][k] = 0.f;
        __builtin_amdgcn_wave_barrier();
        if (part == 0) {
            sdv[sm] = dvm;
            if (mok) { if (VAL) q.dv[m] = dvm; spart[sm][0] = l; spart[sm][1] = VAL ? lv : 0.f; spart[sm][2] = sq; }
        }
        if (aok) { spart[sm][3 + part] = dls; spart[sm][3 + PF_MAX_ACT + part] = mean; }
    }
    __syncthreads();
    pf_block_partials(q, spart, tid);
    pf_head_dh2<NA, PF_NV, VAL>(q, sWm, sWv, sdu, sdv, hp, hv, m, mok, sm, part);
}

// ---------------------------------------------------------------------------------------------------------------------
// input gradient of layer 2: grid (ceil(H1 / 32), 2 nets, ceil(M / 32)); block = a 32 x 32 tile of
//   dh1[m, k] = (sum_n dh2[m, n] W2[k, n]) * relu'(h1[m, k])      the four waves split the 300 columns, partial tiles meet in LDS
// (its own launch: the weight-gradient kernel below updates W2 in place, this one still reads it)
// ---------------------------------------------------------------------------------------------------------------------
template <bool X3>
__global__ __launch_bounds__(256) void ppo_dh1_kernel(const PpoFusedParams q) {
    __shared__ float red[3][16][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lrow = lane & 31, lgrp = lane >> 5;
    const int net = blockIdx.y, H1 = q.H1, H2 = q.H2, M = q.M, k0 = blockIdx.x * 32, m0 = blockIdx.z * 32;
    const float* __restrict__ dh2 = q.dh2 + (long long)net * M * H2;
    const float* __restrict__ W2 = q.theta + pf_off(q, net, 2);
    const float* __restrict__ h1 = q.h1 + (long long)net * M * H1;
    float* dh1 = q.dh1 + (long long)net * M * H1;
    const int nsteps = X3 ? (H2 + 15) / 16 : (H2 + 7) / 8, per = (nsteps + 3) / 4;
    const int sb = wave * per, se = min(nsteps, sb + per);
    const int kk = k0 + lrow;
    const __amdgpu_buffer_rsrc_t rsG = PF_RSRC(dh2, (long long)M * H2 * 4), rsW = PF_RSRC(W2, (long long)H1 * H2 * 4), rsH = PF_RSRC(h1, (long long)M * H1 * 4);
    const unsigned grow = (unsigned)min(m0 + lrow, M - 1) * (unsigned)H2, wrow = (unsigned)min(kk, H1 - 1) * (unsigned)H2, H1u = (unsigned)H1;
    const unsigned col = kk < H1 ? (unsigned)kk * 4u : PF_OOB;
    float hmask[16];                                      // relu'(h1) of this lane's outputs, requested with the operands
    if (wave == 0) {
#pragma unroll
        for (int r = 0; r < 16; ++r) hmask[r] = pf_ld(rsH, (unsigned)(m0 + pf_row(r, lgrp)) * H1u * 4u + col);
    }
    f32x16_t acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    if constexpr (X3) {
        pf_mma_x3_chunked<5>(sb, se,                      // (the same cut-off, per group of 4)
            [&](int s_) { const unsigned n = grow + (unsigned)(s_ * 16 + lgrp * 8); return pf_cat(pf_ld4(rsG, n * 4u), pf_ld4(rsG, (n + 4u) * 4u)); },
            [&](int s_) { const int n = s_ * 16 + lgrp * 8;
                          return pf_cat(pf_ld4(rsW, n < H2 ? (wrow + (unsigned)n) * 4u : PF_OOB), pf_ld4(rsW, n + 4 < H2 ? (wrow + (unsigned)n + 4u) * 4u : PF_OOB)); }, acc);
    } else {
    pf_mma_chunked<10>(sb, se,                            // H2 % 4 == 0; the reduction index past H2 must read zeros on one side: the W2 row is cut off there
        [&](int s_) { return pf_ld4(rsG, (grow + (unsigned)(s_ * 8 + lgrp * 4)) * 4u); },
        [&](int s_) { const int n = s_ * 8 + lgrp * 4; return pf_ld4(rsW, n < H2 ? (wrow + (unsigned)n) * 4u : PF_OOB); }, acc);
    }
    if (wave > 0) {
#pragma unroll
        for (int r = 0; r < 16; ++r) red[wave - 1][r][lane] = acc[r];
    }
    __syncthreads();
    if (wave == 0) {
        const __amdgpu_buffer_rsrc_t rsO = PF_RSRC(q.dh1 + (long long)net * M * H1, (long long)M * H1 * 4);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float v = ((acc[r] + red[0][r][lane]) + (red[1][r][lane] + red[2][r][lane]));
            pf_st(rsO, (unsigned)(m0 + pf_row(r, lgrp)) * H1u * 4u + col, hmask[r] > 0.f ? v : 0.f);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// every weight / bias gradient of both nets (+ single rank: its TF-Adam update) as independent 32 x 32 tiles, one WAVE per tile:
//   dW[k, n] = sum_m X[m, k] G[m, n]        X / G = h1 / dh2 (layer 2), states / dh1 (layer 1), h2 / dhead (head: n < A)
//   tiles of a layer's first 32 rows also produce the bias gradient (column sums of G: one more MFMA per step against all-ones rows)
// grid ceil(tiles / 4) blocks of 4 waves; the last block's spare wave finalises the loss scalars and logstd.  All rows of the minibatch are
// summed inside the wave (M <= 256 on this path), so the update is applied to the tile straight from the accumulators.
// ---------------------------------------------------------------------------------------------------------------------
template <bool FUSE, bool X3>
__global__ __launch_bounds__(256) void ppo_wgrad_kernel(const PpoFusedParams q) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lrow = lane & 31, lgrp = lane >> 5;
    const int H1 = q.H1, H2 = q.H2, M = q.M;
    const int KT1 = (q.kin + 31) / 32, NT1 = (H1 + 31) / 32, KT2 = NT1, NT2 = (H2 + 31) / 32, KTH = NT2;
    const int per_net = KT2 * NT2 + KT1 * NT1 + KTH;
    int t = blockIdx.x * 4 + wave;
    const bool split = !FUSE && q.m_chunk > 0;            // large minibatches: blockIdx.y = row chunk
    float* const gb = split ? q.gslab + (long long)blockIdx.y * q.gslab_stride : q.grads;      // where this wave's gradients go: the chunk's slab (every element of a slab
                                                                                               // is written by exactly one wave; an ordered pass adds the slabs) or the buffer
    const int spare = q.n_wnets * per_net;                // (n_wnets: 2, or 1 for the policy-only clone step -- net 0's tiles, then the spare wave)
    if (t == spare && blockIdx.y != 0) return;
    if (t == spare) {                               // spare wave: loss scalars + logstd (fixed block order: deterministic)
        // lane k sums column k of the per-block partials (one load chain per lane instead of PF_NPART chains on lane 0: this wave's latency was
        // the kernel's duration), lane 0 collects them with shuffles; exp / log through the hardware units (arguments O(1), ~1e-7 relative)
        float col = 0.f;
        if (lane < PF_NPART) for (int b = 0; b < q.n_loss_blocks; ++b) col += q.partial[(long long)b * PF_NPART + lane];
        else if (lane == PF_NPART && q.kl_on) for (int b = 0; b < q.n_loss_blocks; ++b) col += q.kl_partial[b];      // the KL penalty's block sums, on a lane of their own
        else if (lane > PF_NPART && lane <= PF_NPART + 2 && q.m_ppo) for (int b = 0; b < q.n_loss_blocks; ++b) col += q.demo_partial[(long long)b * 2 + (lane - PF_NPART - 1)];      // the demonstration term's two
        const float kl_sum = __shfl(col, PF_NPART, 64);
        const float demo_l = __shfl(col, PF_NPART + 1, 64), demo_sq = __shfl(col, PF_NPART + 2, 64);
        float sum[PF_NPART];
#pragma unroll
        for (int k = 0; k < PF_NPART; ++k) sum[k] = __shfl(col, k, 64);
        const float ls_l = lane < q.A ? q.theta[q.off[6] + lane] : 0.f;      // logstd[a] on lane a
        const float sd_l = __expf(ls_l);
        float ent = 0.f, sd[PF_MAX_ACT];
#pragma unroll
        for (int a = 0; a < PF_MAX_ACT; ++a) { sd[a] = __shfl(sd_l, a, 64); if (a < q.A) ent += 0.5f + PF_HALF_LOG_2PI + __logf(sd[a]); }
        if (lane != 0) return;
        const float pl = sum[0] * q.inv_m, vl = sum[1] * q.inv_m * q.value_scale, el = ent * q.entropy_scale;
        float* L = q.losses;                               // [0..4] policy, value, entropy, total, mean ratio ; [5..5+A) mean action_mean ; [5+A..5+2A) std
        float tot = q.clone ? pl + vl : -pl + vl - el;
        L[0] = pl; L[1] = vl; L[2] = el; L[3] = tot; L[4] = sum[2] * q.inv_m;      // (clone step: [clone_loss, value_loss, 0, loss, mean_sq_error])
#pragma unroll
        for (int a = 0; a < PF_MAX_ACT; ++a) if (a < q.A) { L[5 + a] = sum[3 + PF_MAX_ACT + a] * q.inv_m; L[5 + q.A + a] = sd[a]; }
        if (q.kl_on) {                                    // [5+2A] mean KL(pi_old || pi), [5+2A+1] beta x that, which the total loss also takes
            const float klm = kl_sum * q.inv_m, pen = q.kl_coef * klm;
            tot = (-pl + vl - el) + pen;
            L[5 + 2 * q.A] = klm; L[5 + 2 * q.A + 1] = pen; L[3] = tot;
        }
        if (q.m_ppo) {                                    // the demonstration term: [demo_loss, c_d demo_loss, mean_sq_error] to a buffer of its own; the total takes the weighted term
            const float dlm = demo_l * q.inv_m_demo, dw = q.demo_coef * dlm;
            q.demo_out[0] = dlm; q.demo_out[1] = dw; q.demo_out[2] = demo_sq * q.inv_m_demo; L[3] = tot + dw;
        }
        // the entropy term is state independent: under data parallelism grad_scale = local_M / global_M shares it across the ranks
#pragma unroll
        for (int a = 0; a < PF_MAX_ACT; ++a) if (a < q.A) pf_emit<FUSE>(q, q.off[6] + a, sum[3 + a] - q.entropy_scale * q.grad_scale, gb);
        return;
    }
    if (t > spare) return;
    const int net = t >= per_net ? 1 : 0;
    t -= net * per_net;
    // ---- which tile ----
    const float* __restrict__ X; const float* __restrict__ G; int ldx, ldg, Kx, Ng, ldw, kt, nt, kvalid; long long oW, ob;
    if (t < KT2 * NT2) {                                  // layer 2
        kt = t / NT2; nt = t - kt * NT2;
        X = q.h1 + (long long)net * M * H1; ldx = H1; Kx = H1; G = q.dh2 + (long long)net * M * H2; ldg = H2; Ng = H2;
        oW = pf_off(q, net, 2); ob = pf_off(q, net, 3); ldw = H2; kvalid = H1;
    } else if (t < KT2 * NT2 + KT1 * NT1) {               // layer 1 (rows din .. kin-1 of W1 are the zero padding: their gradient stays 0)
        t -= KT2 * NT2; kt = t / NT1; nt = t - kt * NT1;
        X = q.row_idx ? q.s_gath : q.states; ldx = q.din; Kx = q.din; G = q.dh1 + (long long)net * M * H1; ldg = H1; Ng = H1;
        oW = pf_off(q, net, 0); ob = pf_off(q, net, 1); ldw = H1; kvalid = q.kin;
    } else {                                              // head kernel [H2, A]
        kt = t - KT2 * NT2 - KT1 * NT1; nt = 0;
        X = q.h2 + (long long)net * M * H2; ldx = H2; Kx = H2; const int A = net == 0 ? q.A : 1;
        G = net == 0 ? q.du : q.dv; ldg = A; Ng = A;
        oW = pf_off(q, net, 4); ob = pf_off(q, net, 5); ldw = A; kvalid = H2;
    }
    const int k = kt * 32 + lrow, n = nt * 32 + lrow;
    const bool nok = n < Ng;
    // descriptors: X / G end with the minibatch (rows past M read 0.0), a column past the tensor is sent past the descriptor; the weight tile's
    // descriptor ends at row Kx, so the optimiser state of rows past it reads 0.0 and their stores are dropped
    const __amdgpu_buffer_rsrc_t rsX = PF_RSRC(X, (long long)M * ldx * 4), rsG = PF_RSRC(G, (long long)M * ldg * 4);
    const unsigned xcol = k < Kx ? (unsigned)k * 4u : PF_OOB, gcol = nok ? (unsigned)n * 4u : PF_OOB;
    const unsigned ldxb = (unsigned)ldx * 4u, ldgb = (unsigned)ldg * 4u, ldwb = (unsigned)ldw * 4u;
    const long long wbytes = (long long)Kx * ldw * 4;
    const __amdgpu_buffer_rsrc_t rsP = PF_RSRC(q.theta + oW, wbytes), rsM = PF_RSRC(q.adam_m + oW, wbytes), rsV = PF_RSRC(q.adam_v + oW, wbytes);
    // the tile's optimiser state is requested together with the operands (FUSE): one memory round trip for the whole wave
    float pw[16], pm[16], pv[16];
    if constexpr (FUSE) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const unsigned off = (unsigned)(kt * 32 + pf_row(r, lgrp)) * ldwb + gcol;
            pw[r] = pf_ld(rsP, off); pm[r] = pf_ld(rsM, off); pv[r] = pf_ld(rsV, off);
        }
    }
    f32x16_t acc, accb;
#pragma unroll
    for (int r = 0; r < 16; ++r) { acc[r] = 0.f; accb[r] = 0.f; }
    const int m_beg = split ? (int)blockIdx.y * q.m_chunk : 0, m_end = split ? min(M, m_beg + q.m_chunk) : M;
    if constexpr (X3) {                                   // 32 rows per round as below: two k-blocks of 16, rows 16 s + 8 h + j on lane half h
        const int mblocks = (m_end + 15) / 16;
        for (int s0 = m_beg / 16; s0 < mblocks; s0 += 2) {
            f32x8_t a[2], b[2];
#pragma unroll
            for (int u = 0; u < 2; ++u)
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const unsigned mm = (unsigned)((s0 + u) * 16 + lgrp * 8 + e);
                    a[u][e] = pf_ld(rsX, mm * ldxb + xcol);
                    b[u][e] = pf_ld(rsG, mm * ldgb + gcol);
                }
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                pf_mma_x3(a[u], b[u], acc);
                if (kt == 0) pf_colsum_x3(b[u], accb);
            }
        }
    } else {
    const int msteps = (m_end + 7) / 8;
    for (int s0 = m_beg / 8; s0 < msteps; s0 += 4) {
        f32x4 a[4], b[4];
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const unsigned mm = (unsigned)((s0 + u) * 8 + lgrp * 4 + e);
                a[u][e] = pf_ld(rsX, mm * ldxb + xcol);
                b[u][e] = pf_ld(rsG, mm * ldgb + gcol);
            }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            pf_mma4(a[u], b[u], acc);
            if (kt == 0) pf_mma4(f32x4{1.f, 1.f, 1.f, 1.f}, b[u], accb);          // all-ones rows: every output row = column sums of G
        }
    }
    }
    if (!nok) return;
    if constexpr (FUSE) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const unsigned off = (unsigned)(kt * 32 + pf_row(r, lgrp)) * ldwb + gcol;
            float mm_ = pm[r], vv_ = pv[r];
            mm_ += (acc[r] - mm_) * q.omb1; vv_ += (acc[r] * acc[r] - vv_) * q.omb2;
            pf_st(rsM, off, mm_); pf_st(rsV, off, vv_);
            pf_st(rsP, off, pw[r] - (mm_ * q.alpha) / (sqrtf(vv_) + q.epsilon));
        }
    } else {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int kr = kt * 32 + pf_row(r, lgrp);
            const long long idx = oW + (long long)kr * ldw + n;
            if (kr < Kx) gb[idx] = acc[r];
            else if (kr < kvalid) gb[idx] = 0.f;
        }
    }
    if (kt == 0 && lgrp == 0) pf_emit<FUSE>(q, ob + n, accb[0], gb);
}

// ---------------------------------------------------------------------------------------------------------------------
// heads of PPO.predict (ppo.py:47,58-62,231-251) on the trunks of nets 0 / 1: action = clip(mean + exp(logstd) noise, low, high) or the mean,
// value = h2_v Wv + bv.  with logp_out: log pi(a | s) of GIVEN actions under net `lp_net` (0 policy, 2 old policy) instead (the cache of
// log pi_old for a whole horizon batch).  grid ceil(M / 32) blocks; 8 threads per sample.
// ---------------------------------------------------------------------------------------------------------------------
// LG: log2 of the threads per sample: 3 (32 samples per block) for batches, 6 (a wave per sample: 5 instead of 38 dependent steps over the 300 columns)
// for the handful of samples of an interactive predict
template <int NA, int LG>
__global__ __launch_bounds__(256) void ppo_predict_head_kernel(const PpoFusedParams q, const float* __restrict__ noise, int greedy,
                                                               float* __restrict__ action, float* __restrict__ value, float* __restrict__ logp_out, int lp_net) {
    constexpr int TPS = 1 << LG, SPB = 256 / TPS;
    const int tid = threadIdx.x, m0 = blockIdx.x * SPB, A = q.A, H2 = q.H2;
    const int sm = tid >> LG, part = tid & (TPS - 1), m = m0 + sm;
    const float* th = lp_net == 2 ? q.theta_old : q.theta;
    const float* Wm = th + q.off[4]; const float* bm = th + q.off[5]; const float* logstd = th + q.off[6];
    const float* Wv = q.theta + q.off[11]; const float* bv = q.theta + q.off[12];
    const float* h2p = q.h2 + (long long)(logp_out ? (lp_net == 2 ? 2 : 0) : 0) * q.M * H2; const float* h2v = q.h2 + (long long)q.M * H2;
    float au[NA], av;
    pf_head_sums_strided<NA, TPS>(h2p + (long long)m * H2, h2v + (long long)m * H2, Wm, Wv, m < q.M, !logp_out, part, H2, A, au, av);
    if (part != 0 || m >= q.M) return;
    float lp = 0.f;
    _Pragma("unroll") for (int a = 0; a < NA; ++a) if (a < A) {
        const float lo = q.low[a], hi = q.high[a];
        const float mean = pf_mean_libm(au[a], bm[a], lo, hi);
        if (logp_out) {
            lp += pf_logp_term_libm(q.actions[(long long)m * A + a], mean, logstd[a]);
            if (q.mean_old_out) q.mean_old_out[(long long)m * A + a] = mean;      // (mi_ppo_old_policy_cache: the means the KL penalty reads)
        } else {
            if (q.mean_out) q.mean_out[(long long)m * A + a] = mean;
            float act = mean;
            if (!greedy) act = fminf(fmaxf(mean + expf(logstd[a]) * noise[(long long)m * A + a], lo), hi);
            action[(long long)m * A + a] = act;
        }
    }
    if (logp_out) logp_out[m] = lp; else value[m] = av + bv[0];
}

// ---------------------------------------------------------------------------------------------------------------------
// update diagnostics (mi_ppo_update_stats_idx): heads of the CURRENT policy and value net on the trunks of nets 0 / 1, and the per-sample terms of the
// MI_PPO_N_STATS running sums in double precision.  grid ceil(M / 32) blocks; 8 threads per sample, sample m = table row row_idx[m] (clamped).
//   lp = log pi(a | s) under theta in the strided form of ppo_predict_head_kernel<NA, 3>'s log-probability path (the contracts: ppo_head.hpp), so that with
//        theta == theta_old it is the cached logp_old bit for bit;  v = h2_v Wv + bv in that kernel's order
//   d = lp - logp_old, r = exp(d), ret = returns: terms 1, d, r - 1 - d (k3), |r - 1| > clip_eps, r, ret, ret^2, ret - v, (ret - v)^2
// Ordered reduction, no atomics: pf_ordered_block_sum stores this block's row of `scratch`; ppo_stats_reduce_kernel adds the rows in block order.
// ---------------------------------------------------------------------------------------------------------------------
constexpr int PF_NSTATS = MI_PPO_N_STATS;
template <int NA>
__global__ __launch_bounds__(256) void ppo_update_stats_head_kernel(const PpoFusedParams q, double* __restrict__ scratch, float* __restrict__ logp_new_out, float* __restrict__ value_out) {
    __shared__ double swave[4][PF_NSTATS];
    const int tid = threadIdx.x, m0 = blockIdx.x * 32, A = q.A, H2 = q.H2;
    const int sm = tid >> 3, part = tid & 7, m = m0 + sm;
    const float* Wm = q.theta + q.off[4]; const float* bm = q.theta + q.off[5]; const float* logstd = q.theta + q.off[6];
    const float* Wv = q.theta + q.off[11]; const float* bv = q.theta + q.off[12];
    const float* h2p = q.h2; const float* h2v = q.h2 + (long long)q.M * H2;
    float au[NA], av;
    pf_head_sums_strided<NA, 8>(h2p + (long long)m * H2, h2v + (long long)m * H2, Wm, Wv, m < q.M, true, part, H2, A, au, av);
    double term[PF_NSTATS];
#pragma unroll
    for (int k = 0; k < PF_NSTATS; ++k) term[k] = 0.0;
    if (part == 0 && m < q.M) {
        const long long mr = min(max(q.row_idx[m], 0), q.n_rows - 1);
        float lp = 0.f;
        _Pragma("unroll") for (int a = 0; a < NA; ++a) if (a < A) {
            lp += pf_logp_term_libm(q.actions[mr * A + a], pf_mean_libm(au[a], bm[a], q.low[a], q.high[a]), logstd[a]);
        }
        const float v = av + bv[0];
        if (logp_new_out) logp_new_out[mr] = lp;
        if (value_out) value_out[mr] = v;
        const double d = (double)lp - (double)q.logp_old[mr];
        const double r = exp(d);
        const double ret = (double)q.returns[mr], e = ret - (double)v;
        term[0] = 1.0; term[1] = d; term[2] = (r - 1.0) - d; term[3] = fabs(r - 1.0) > (double)q.clip_eps ? 1.0 : 0.0; term[4] = r;
        term[5] = ret; term[6] = ret * ret; term[7] = e; term[8] = e * e;
    }
    pf_ordered_block_sum<PF_NSTATS>(term, swave, scratch, tid);
}

// ---------------------------------------------------------------------------------------------------------------------
// exact-KL statistics (mi_ppo_kl_stats_idx): the head of the CURRENT policy on the trunk of net 0, and per sample the closed-form KL(pi_old || pi_theta) of the
// diagonal Gaussians in double precision from the fp32 means (this pass: the strided form of ppo_predict_head_kernel<NA, 3>, ppo_head.hpp, so that with
// theta == theta_old the mean is the cached one bit for bit and the KL is 0; old: q.mean_old[row]) and the two log-stds:
//   KL[m] = sum_a d + expm1(-2 d) / 2 + D^2 / (2 sigma^2) ,  d = ls - lso, D = mu - mu_o, sigma = exp(ls)
// terms 1, KL, KL^2, sum_a D^2 / (2 sigma^2) (the mean part).  grid ceil(M / 32) blocks; 8 threads per sample, sample m = table row row_idx[m] (clamped).  The
// reduction is that of ppo_update_stats_head_kernel.
// ---------------------------------------------------------------------------------------------------------------------
constexpr int PF_NKLSTATS = MI_PPO_N_KL_STATS;
template <int NA>
__global__ __launch_bounds__(256) void ppo_kl_stats_head_kernel(const PpoFusedParams q, double* __restrict__ scratch) {
    __shared__ double swave[4][PF_NKLSTATS];
    const int tid = threadIdx.x, m0 = blockIdx.x * 32, A = q.A, H2 = q.H2;
    const int sm = tid >> 3, part = tid & 7, m = m0 + sm;
    const float* Wm = q.theta + q.off[4]; const float* bm = q.theta + q.off[5]; const float* logstd = q.theta + q.off[6]; const float* logstd_o = q.theta_old + q.off[6];
    const float* h2p = q.h2;
    float au[NA], av;                                     // (av: no value net here)
    pf_head_sums_strided<NA, 8>(h2p + (long long)m * H2, nullptr, Wm, nullptr, m < q.M, false, part, H2, A, au, av);
    double term[PF_NKLSTATS];
#pragma unroll
    for (int k = 0; k < PF_NKLSTATS; ++k) term[k] = 0.0;
    if (part == 0 && m < q.M) {
        const long long mr = min(max(q.row_idx[m], 0), q.n_rows - 1);
        double kl = 0.0, mp = 0.0;
        _Pragma("unroll") for (int a = 0; a < NA; ++a) if (a < A) {
            const float mean = pf_mean_libm(au[a], bm[a], q.low[a], q.high[a]);
            const double ls = (double)logstd[a], d = ls - (double)logstd_o[a], dm = (double)mean - (double)q.mean_old[mr * A + a];
            const double qh = 0.5 * dm * dm * exp(-2.0 * ls);      // D^2 / (2 sigma^2)
            kl += d + 0.5 * expm1(-2.0 * d) + qh;
            mp += qh;
        }
        term[0] = 1.0; term[1] = kl; term[2] = kl * kl; term[3] = mp;
    }
    pf_ordered_block_sum<PF_NKLSTATS>(term, swave, scratch, tid);
}

// ---------------------------------------------------------------------------------------------------------------------
// values of table rows (mi_ppo_values_idx): the value head of the CURRENT value net alone, on a trunk that ran the value net as net 0 -- the caller's parameter
// block has off[0..3] = off[7..10] and n_nets = 1, so h2 slot 0 holds the value net's activations; Wv / bv stay at off[11] / off[12].  grid ceil(M / 32) blocks; 8
// threads per sample, ppo_update_stats_head_kernel's part / row split and, through pf_head_sums_strided, its order of operations: the stored value is that
// kernel's value_out bit for bit (the contracts: ppo_head.hpp).  Sample m is table row row_idx[m] (nullptr: m) and its value goes to values_out[that row]; a row
// outside [0, n_rows) stores NOTHING (the statistics head clamps the store; layer 1 clamped the loads).  No LDS, no atomics, no reduction behind it.
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ppo_values_head_kernel(const PpoFusedParams q, float* __restrict__ values_out) {
    const int tid = threadIdx.x, m0 = blockIdx.x * 32, H2 = q.H2;
    const int sm = tid >> 3, part = tid & 7, m = m0 + sm;
    const float* Wv = q.theta + q.off[11]; const float* bv = q.theta + q.off[12];
    const float* h2v = q.h2 + (long long)m * H2;          // (slot 0: see above)
    float au[1], av;                                      // (A = 0: no policy sums are formed)
    pf_head_sums_strided<1, 8>(h2v, h2v, Wv, Wv, m < q.M, true, part, H2, 0, au, av);
    if (part != 0 || m >= q.M) return;
    const int row = q.row_idx ? q.row_idx[m] : m;
    if (row < 0 || row >= q.n_rows) return;
    values_out[row] = av + bv[0];
}

// ---------------------------------------------------------------------------------------------------------------------
// log pi_theta(a | s) of table rows (mi_ppo_logp_idx): the policy head of the CURRENT parameters alone, on the trunk of net 0 -- the twin of ppo_values_head_kernel
// for the policy side, and the log-probability path of ppo_update_stats_head_kernel without the value net, the double-precision terms and the reduction.  grid
// ceil(M / 32) blocks; 8 threads per sample, that kernel's part / row split and, through pf_head_sums_strided / pf_mean_libm / pf_logp_term_libm and the serial sum
// over a = 0, 1, .., its order of operations: the stored float is that kernel's logp_new_out bit for bit, and with theta == theta_old the cache of mi_ppo_logp_old
// (the fifth contract: ppo_head.hpp).  Sample m is table row row_idx[m] (nullptr: m); q.actions is gathered by that row and the result goes to logp_out[that
// row]; a row outside [0, n_rows) stores NOTHING (its loads are clamped, as layer 1 clamped the state's).  No LDS, no atomics, no reduction behind it.
// ---------------------------------------------------------------------------------------------------------------------
template <int NA>
__global__ __launch_bounds__(256) void ppo_logp_head_kernel(const PpoFusedParams q, float* __restrict__ logp_out) {
    const int tid = threadIdx.x, m0 = blockIdx.x * 32, A = q.A, H2 = q.H2;
    const int sm = tid >> 3, part = tid & 7, m = m0 + sm;
    const float* Wm = q.theta + q.off[4]; const float* bm = q.theta + q.off[5]; const float* logstd = q.theta + q.off[6];
    float au[NA], av;                                     // (av: no value net here)
    pf_head_sums_strided<NA, 8>(q.h2 + (long long)m * H2, nullptr, Wm, nullptr, m < q.M, false, part, H2, A, au, av);
    if (part != 0 || m >= q.M) return;
    const int row = q.row_idx ? q.row_idx[m] : m;
    const long long mr = min(max(row, 0), q.n_rows - 1);
    float lp = 0.f;
    _Pragma("unroll") for (int a = 0; a < NA; ++a) if (a < A) {
        lp += pf_logp_term_libm(q.actions[mr * A + a], pf_mean_libm(au[a], bm[a], q.low[a], q.high[a]), logstd[a]);
    }
    if (row < 0 || row >= q.n_rows) return;
    logp_out[row] = lp;
}

// ---------------------------------------------------------------------------------------------------------------------
// dual-clip diagnostics (mi_ppo_dual_clip_stats): what the dual-clipped surrogate of ppo_head_loss_body did to M rows row_idx[m] (clamped) of three fp32 tables --
// lp = log pi_theta(a | s) (the logp_new_out table of mi_ppo_update_stats_idx), lpo = the cached log pi_old, A = the advantage the steps gathered.  No engine, no
// network: one thread per sample, 256 samples per block.  The CLASS of a sample is formed in fp32 as the step forms it, operation for operation --
//   r = __expf(lp - lpo), s1 = r A, s2 = clamp(r, 1 - eps, 1 + eps) A, s = min(s1, s2), dual-clipped iff A < 0 and c A > s
// -- so the counts say what the step did; the two SUMS are taken in double from the fp32 inputs (r = exp((double)lp - (double)lpo)), like the other statistics
// passes' terms.  terms 1, A < 0, dual-clipped, s' (c A on a dual-clipped sample, else s), s.  Ordered reduction, no atomics: the xor rounds 1, 2, 4 here and
// pf_ordered_block_sum's 8, 16, 32 are a wave's whole tree; ppo_stats_reduce_kernel adds the block rows in block order.  Rows that row_idx does not name are not read.
// ---------------------------------------------------------------------------------------------------------------------
constexpr int PF_NDCSTATS = MI_PPO_N_DUAL_CLIP_STATS;
__global__ __launch_bounds__(256) void ppo_dual_clip_stats_kernel(const float* __restrict__ logp_new, const float* __restrict__ logp_old, const float* __restrict__ advantage,
                                                                  const int* __restrict__ row_idx, int n_rows, int M, float clip_eps, float dual_clip, double* __restrict__ scratch) {
    __shared__ double swave[4][PF_NDCSTATS];
    const int tid = threadIdx.x, m = blockIdx.x * 256 + tid;
    double term[PF_NDCSTATS];
#pragma unroll
    for (int k = 0; k < PF_NDCSTATS; ++k) term[k] = 0.0;
    if (m < M) {
        const long long mr = min(max(row_idx[m], 0), n_rows - 1);
        const float lp = logp_new[mr], lpo = logp_old[mr], ad = advantage[mr];
        const float r = __expf(lp - lpo);
        const float rc = fminf(fmaxf(r, 1.0f - clip_eps), 1.0f + clip_eps);
        const float s1 = r * ad, s2 = rc * ad;
        const bool dual = ad < 0.f && dual_clip * ad > fminf(s1, s2);
        const double rd = exp((double)lp - (double)lpo), add = (double)ad;
        const double rcd = fmin(fmax(rd, 1.0 - (double)clip_eps), 1.0 + (double)clip_eps);
        const double sd = fmin(rd * add, rcd * add);
        term[0] = 1.0; term[1] = ad < 0.f ? 1.0 : 0.0; term[2] = dual ? 1.0 : 0.0; term[3] = dual ? (double)dual_clip * add : sd; term[4] = sd;
    }
#pragma unroll
    for (int k = 0; k < PF_NDCSTATS; ++k) {
#pragma unroll
        for (int o = 1; o < 8; o <<= 1) term[k] += __shfl_xor(term[k], o, 64);
    }
    pf_ordered_block_sum<PF_NDCSTATS>(term, swave, scratch, tid);
}

}  // namespace mi

using namespace mi;

// shapes the fused kernels are built for (checked BEFORE anything is launched; the engine falls back to the per-layer path otherwise)
bool mi_ppo_fused_shape_in_range(int A, int H2, int kin) { return A >= 1 && A <= PF_MAX_ACT && H2 <= PF_H2MAX && H2 % 4 == 0 && kin <= 96; }
// ... and with wide inputs switched on (mi_ppo_set_wide_inputs): the same limits on A and H2, kin <= 1024
constexpr int PF_KIN_WIDE = 1024;
bool mi_ppo_fused_shape_in_wide_range(int A, int H2, int kin) { return A >= 1 && A <= PF_MAX_ACT && H2 <= PF_H2MAX && H2 % 4 == 0 && kin <= PF_KIN_WIDE; }
static int pf_check_shape(const PpoFusedParams& q, const char* who) {
    static thread_local char msg[224];
    if (!(q.wide ? mi_ppo_fused_shape_in_wide_range(q.A, q.H2, q.kin) : mi_ppo_fused_shape_in_range(q.A, q.H2, q.kin))) {
        snprintf(msg, sizeof(msg), "%s: shape outside the fused kernels' range (1 <= num_actions <= 8, H2 <= 320 and a multiple of 4, inputs <= %d)", who, q.wide ? PF_KIN_WIDE : 96);
        return mi_fail(MI_ERR_SHAPE, msg);
    }
    // the buffer descriptors take their size as an int and the kernels form 32-bit byte offsets: a state table (n_rows rows with a row index, else the M rows of the
    // call), the padded minibatch of the engine's max_batch rows and a layer-1 kernel stay below 2 GiB
    const long long lim = 1ll << 31, rows = q.row_idx ? q.n_rows : q.M;
    if (rows * q.din * 4 >= lim || (long long)(q.max_batch > q.M ? q.max_batch : q.M) * q.kin * 4 >= lim || (long long)q.kin * q.H1 * 4 >= lim) {
        snprintf(msg, sizeof(msg), "%s: a state table of %lld rows x %d inputs (or max_batch x the padded width, or the layer-1 kernel) reaches 2 GiB: the fused kernels address it with 32-bit byte offsets",
                 who, rows, q.din);
        return mi_fail(MI_ERR_SHAPE, msg);
    }
    return MI_OK;
}

// the predict / logp_old / statistics heads take their NA = 2 instantiation up to two actions, A = 1 included -- unlike the loss and clone kernels of the step
// (pf_step_head_kernel), which take theirs for A == 2 only
template <class K> static K pf_na_pick(int A, K k2, K k8) { return A <= 2 ? k2 : k8; }

int mi_ppo_fused_predict(hipStream_t st, PpoFusedParams& q, const float* noise, int greedy, float* action, float* value) {
    { const int rc0 = pf_check_shape(q, "ppo fused predict"); if (rc0 != MI_OK) return rc0; }
    q.n_nets = 2;
    int rc = mi_ppo_fused_trunks(st, q, false);            // (PPO.predict stays exact fp32 in every precision mode)
    if (rc != MI_OK) return rc;
    if (q.M <= 8)                                         // a wave per sample
        hipLaunchKernelGGL(pf_na_pick(q.A, ppo_predict_head_kernel<2, 6>, ppo_predict_head_kernel<PF_MAX_ACT, 6>), dim3((q.M + 3) / 4), dim3(256), 0, st, q, noise, greedy, action, value, (float*)nullptr, 0);
    else
        hipLaunchKernelGGL(pf_na_pick(q.A, ppo_predict_head_kernel<2, 3>, ppo_predict_head_kernel<PF_MAX_ACT, 3>), dim3((q.M + 31) / 32), dim3(256), 0, st, q, noise, greedy, action, value, (float*)nullptr, 0);
    return mi_check_launch("ppo_predict_head");
}

// log pi_old(a | s) of M samples (theta_old's trunk in net slot 2); x3: the trunks in the split-bf16 form, as in the step of that mode
int mi_ppo_fused_logp_old(hipStream_t st, PpoFusedParams& q, float* out, bool x3) {
    // only net 2 is needed: run the trunk kernels over the grid's net range [2, 3) by offsetting nothing -- the kernels index nets by blockIdx.y,
    // so all three are computed (M x 1.2 MFLOP, once per horizon batch)
    { const int rc0 = pf_check_shape(q, "ppo fused logp_old"); if (rc0 != MI_OK) return rc0; }
    q.n_nets = 3;
    int rc = mi_ppo_fused_trunks(st, q, x3);
    if (rc != MI_OK) return rc;
    hipLaunchKernelGGL(pf_na_pick(q.A, ppo_predict_head_kernel<2, 3>, ppo_predict_head_kernel<PF_MAX_ACT, 3>), dim3((q.M + 31) / 32), dim3(256), 0, st, q, (const float*)nullptr, 1, (float*)nullptr, (float*)nullptr, out, 2);
    return mi_check_launch("ppo_logp_old");
}

// update diagnostics of M gathered rows under the current theta (q.row_idx / n_rows / actions / returns / logp_old set by the caller): the policy and value trunks,
// the statistics head, the ordered sum of its block rows into stats.  Nothing but the activation workspace, scratch, stats and the two optional tables is written.
int mi_ppo_fused_update_stats(hipStream_t st, PpoFusedParams& q, int accumulate, double* scratch, double* stats, float* logp_new_out, float* value_out, bool x3) {
    { const int rc0 = pf_check_shape(q, "ppo fused update stats"); if (rc0 != MI_OK) return rc0; }
    q.n_nets = 2;
    q.s_gath = nullptr;                                   // (no filter gradient behind this pass: layer 1 gathers its operand rows and leaves no copy)
    int rc = mi_ppo_fused_trunks(st, q, x3);
    if (rc != MI_OK) return rc;
    const int nb = (q.M + 31) / 32;
    hipLaunchKernelGGL(pf_na_pick(q.A, ppo_update_stats_head_kernel<2>, ppo_update_stats_head_kernel<PF_MAX_ACT>), dim3(nb), dim3(256), 0, st, q, scratch, logp_new_out, value_out);
    hipLaunchKernelGGL(ppo_stats_reduce_kernel<PF_NSTATS>, dim3(1), dim3(64), 0, st, (const double*)scratch, nb, accumulate, stats);
    return mi_check_launch("ppo_update_stats");
}

// exact KL(pi_old || pi_theta) sums of M gathered rows under the current theta (q.row_idx / n_rows / mean_old set by the caller): the policy trunk alone, the
// statistics head, the ordered sum of its block rows into stats.  Nothing but the activation workspace, scratch and stats is written.
int mi_ppo_fused_kl_stats(hipStream_t st, PpoFusedParams& q, int accumulate, double* scratch, double* stats, bool x3) {
    { const int rc0 = pf_check_shape(q, "ppo fused kl stats"); if (rc0 != MI_OK) return rc0; }
    q.n_nets = 1;                                         // (net 0: the policy)
    q.s_gath = nullptr;
    int rc = mi_ppo_fused_trunks(st, q, x3);
    if (rc != MI_OK) return rc;
    const int nb = (q.M + 31) / 32;
    hipLaunchKernelGGL(pf_na_pick(q.A, ppo_kl_stats_head_kernel<2>, ppo_kl_stats_head_kernel<PF_MAX_ACT>), dim3(nb), dim3(256), 0, st, q, scratch);
    hipLaunchKernelGGL(ppo_stats_reduce_kernel<PF_NKLSTATS>, dim3(1), dim3(64), 0, st, (const double*)scratch, nb, accumulate, stats);
    return mi_check_launch("ppo_kl_stats");
}

// the dual-clip diagnostics (include/mi355_carla.h): no engine, two launches, nothing but scratch and stats is written
extern "C" long long mi_ppo_dual_clip_stats_scratch_doubles(int M) { return (long long)MI_PPO_N_DUAL_CLIP_STATS * (M < 1 ? 1 : (M + 255) / 256); }

extern "C" int mi_ppo_dual_clip_stats(void* stream, const float* logp_new, const float* logp_old, const float* advantage, const int* row_idx, int n_rows, int M,
                                      float clip_eps, float dual_clip, int accumulate, double* scratch, double* stats) {
    if (M < 1 || n_rows < 1) return mi_fail(MI_ERR_ARG, "mi_ppo_dual_clip_stats: empty input (M >= 1, n_rows >= 1)");
    if (!logp_new || !logp_old || !advantage || !row_idx || !scratch || !stats) return mi_fail(MI_ERR_ARG, "mi_ppo_dual_clip_stats: missing buffers");
    if (!(clip_eps > 0.f) || !(clip_eps <= 3.402823466e+38f)) return mi_fail(MI_ERR_ARG, "mi_ppo_dual_clip_stats: clip_eps is a finite float > 0");
    if (!(dual_clip > 1.f)) return mi_fail(MI_ERR_ARG, "mi_ppo_dual_clip_stats: dual_clip is a float > 1 or +inf");
    if (accumulate != 0 && accumulate != 1) return mi_fail(MI_ERR_ARG, "mi_ppo_dual_clip_stats: accumulate is 0 (store the sums) or 1 (add them to stats)");
    const int nb = (M + 255) / 256;
    hipLaunchKernelGGL(ppo_dual_clip_stats_kernel, dim3(nb), dim3(256), 0, (hipStream_t)stream, logp_new, logp_old, advantage, row_idx, n_rows, M, clip_eps, dual_clip, scratch);
    hipLaunchKernelGGL(ppo_stats_reduce_kernel<PF_NDCSTATS>, dim3(1), dim3(64), 0, (hipStream_t)stream, (const double*)scratch, nb, accumulate, stats);
    return mi_check_launch("ppo_dual_clip_stats");
}

// V(s) of M table rows under the current theta (mi_ppo_values_idx): the value net ALONE.  The trunk kernels number nets by blockIdx.y from 0, so a copy of the
// parameter block with the value net's layer-1 / layer-2 tensors in net 0's places (off[0..3] = off[7..10]) and n_nets = 1 runs it in slot 0 of h1 / h2 without a
// kernel change; the head reads Wv / bv at the untouched off[11] / off[12].  M may exceed the engine's max_batch: chunks of max_batch rows, three launches each
// (row_idx given: the chunk's part of the list against the whole table; else the chunk's rows of states / values_out).  Every chunk is checked before the first
// launch.  Nothing but the activation workspace and values_out is written.
int mi_ppo_fused_values(hipStream_t st, const PpoFusedParams& q0, const int* row_idx, long long n_rows, long long M, float* values_out, bool x3) {
    PpoFusedParams q = q0;
    for (int i = 0; i < 4; ++i) q.off[i] = q0.off[7 + i];
    q.n_nets = 1;
    q.s_gath = nullptr;                                   // (no filter gradient behind this pass)
    const long long mb = q.max_batch;
    // (a table the 32-bit offsets cannot address is refused by pf_check_shape whatever its row count: the int field saturates)
    const int n_rows_i = n_rows > 0x7fffffffll ? 0x7fffffff : (int)n_rows;
    for (long long lo = 0; lo < M; lo += mb) {
        const int m = (int)(M - lo < mb ? M - lo : mb);
        q.M = m;
        if (row_idx) { q.states = q0.states; q.row_idx = row_idx + lo; q.n_rows = n_rows_i; }
        else { q.states = q0.states + lo * q.din; q.row_idx = nullptr; q.n_rows = m; }
        // the first chunk is the largest and every chunk addresses the same table: its check, before the first launch, is the call's
        if (lo == 0) { const int rc0 = pf_check_shape(q, "ppo fused values"); if (rc0 != MI_OK) return rc0; }
        const int rc = mi_ppo_fused_trunks(st, q, x3);
        if (rc != MI_OK) return rc;
        hipLaunchKernelGGL(ppo_values_head_kernel, dim3((m + 31) / 32), dim3(256), 0, st, q, row_idx ? values_out : values_out + lo);
        const int rc2 = mi_check_launch("ppo_values_head");
        if (rc2 != MI_OK) return rc2;
    }
    return MI_OK;
}

// log pi_theta(a | s) of M table rows under the current theta (mi_ppo_logp_idx): the policy net ALONE -- net 0 already, so the parameter block goes in as it is
// with n_nets = 1.  mi_ppo_fused_values' chunk loop and row rules: chunks of max_batch rows, three launches each (row_idx given: the chunk's part of the list
// against the whole tables; else the chunk's rows of states / actions / logp_out); the first chunk's check, before the first launch, is the call's.  Nothing but
// the activation workspace and logp_out is written.
int mi_ppo_fused_logp(hipStream_t st, const PpoFusedParams& q0, const float* actions, const int* row_idx, long long n_rows, long long M, float* logp_out, bool x3) {
    PpoFusedParams q = q0;
    q.n_nets = 1;                                         // (net 0: the policy)
    q.s_gath = nullptr;                                   // (no filter gradient behind this pass)
    const long long mb = q.max_batch;
    const int n_rows_i = n_rows > 0x7fffffffll ? 0x7fffffff : (int)n_rows;
    for (long long lo = 0; lo < M; lo += mb) {
        const int m = (int)(M - lo < mb ? M - lo : mb);
        q.M = m;
        if (row_idx) { q.states = q0.states; q.actions = actions; q.row_idx = row_idx + lo; q.n_rows = n_rows_i; }
        else { q.states = q0.states + lo * q.din; q.actions = actions + lo * q.A; q.row_idx = nullptr; q.n_rows = m; }
        if (lo == 0) { const int rc0 = pf_check_shape(q, "ppo fused logp"); if (rc0 != MI_OK) return rc0; }
        const int rc = mi_ppo_fused_trunks(st, q, x3);
        if (rc != MI_OK) return rc;
        hipLaunchKernelGGL(pf_na_pick(q.A, ppo_logp_head_kernel<2>, ppo_logp_head_kernel<PF_MAX_ACT>), dim3((m + 31) / 32), dim3(256), 0, st, q, row_idx ? logp_out : logp_out + lo);
        const int rc2 = mi_check_launch("ppo_logp_head");
        if (rc2 != MI_OK) return rc2;
    }
    return MI_OK;
}

int mi_ppo_fused_partial_floats(int M) { return ((M + 31) / 32) * PF_NPART; }

// forward only (PPO.predict, the cache of log pi_old): layers 1-2 of `n_nets` nets, then the caller's head kernel; x3: split-bf16 instantiations
int mi_ppo_fused_trunks(hipStream_t st, const PpoFusedParams& q, bool x3) {
    const dim3 g1((q.H1 + 127) / 128, q.n_nets, (q.M + 31) / 32), g2((q.H2 + 31) / 32, q.n_nets, (q.M + 31) / 32);
    const dim3 g1w((q.H1 + 31) / 32, q.n_nets, (q.M + 31) / 32);
    const bool wide_l1 = q.wide == 1 && q.kin > 96;       // (mi_ppo_set_wide_inputs: mode 2 keeps ppo_l1_kernel at every width)
    if (x3) {
        if (wide_l1) hipLaunchKernelGGL(ppo_l1_wide_kernel<true>, g1w, dim3(256), 0, st, q);
        else hipLaunchKernelGGL(ppo_l1_kernel<true>, g1, dim3(256), 0, st, q);
        hipLaunchKernelGGL(ppo_l2_kernel<true>, g2, dim3(256), 0, st, q);
    } else {
        if (wide_l1) hipLaunchKernelGGL(ppo_l1_wide_kernel<false>, g1w, dim3(256), 0, st, q);
        else hipLaunchKernelGGL(ppo_l1_kernel<false>, g1, dim3(256), 0, st, q);
        hipLaunchKernelGGL(ppo_l2_kernel<false>, g2, dim3(256), 0, st, q);
    }
    return mi_check_launch("ppo_fused_trunks");
}

// Measurement aid (round 5; profiles/r05_ppo.md): MI355_PPO_PAD=n issues n trivial one-wave launches behind layer 2 and n behind the layer-1
// input gradient -- 2 n extra dependent kernel boundaries on the step's stream.  (wall(n) - wall(0)) / 2 n is what ONE boundary costs inside THIS launch chain on this
// box, i.e. the most a fusion that removes a boundary can win before it has paid for any recomputation.  Default 0: nothing is launched.
// Compiled only with -DMI355_PPO_PAD_PROBE (HIPCC_EXTRA=-DMI355_PPO_PAD_PROBE python -m mi355.build --force): the production step carries no measurement code.
#ifdef MI355_PPO_PAD_PROBE
__global__ void ppo_boundary_probe_kernel(float* sink) { if (threadIdx.x == 1024) sink[0] = 0.f; }
static int ppo_pad(hipStream_t st, float* sink) {
    const int pad = knob(K_PPO_PAD);
    for (int i = 0; i < pad; ++i) hipLaunchKernelGGL(ppo_boundary_probe_kernel, dim3(1), dim3(64), 0, st, sink);
    return pad ? mi_check_launch("ppo_boundary_probe") : MI_OK;
}
#else
static inline int ppo_pad(hipStream_t, float*) { return MI_OK; }
#endif

// the head / loss kernel of a step.  NA = 2 only for A == 2 (the 16-byte LDS reads of pf_head_sums need exactly two actions; A = 1 runs the general form).
//   behaviour cloning (mi_ppo_clone_step): by returns given (VAL)
//   PPO: by the KL-penalised surrogate (KLP: mi_ppo_train_step_kl) and the clipped value loss (VCLIP: v_old given; mi_ppo_train_step_vclip)
typedef void (*pf_head_kernel_t)(const PpoFusedParams);
static pf_head_kernel_t pf_step_head_kernel(const PpoFusedParams& q) {
    static const pf_head_kernel_t demo_table[8] = {       // the demonstration step (m_ppo > 0): [4 KLP + 2 VCLIP] + (A == 2)
        ppo_head_demo_kernel<PF_MAX_ACT>, ppo_head_demo_kernel<2>, ppo_head_demo_vclip_kernel<PF_MAX_ACT>, ppo_head_demo_vclip_kernel<2>,
        ppo_head_demo_kl_kernel<PF_MAX_ACT>, ppo_head_demo_kl_kernel<2>, ppo_head_demo_kl_vclip_kernel<PF_MAX_ACT>, ppo_head_demo_kl_vclip_kernel<2>};
    if (q.m_ppo) return demo_table[4 * (q.kl_on != 0) + 2 * (q.v_old != nullptr) + (q.A == 2)];
    static const pf_head_kernel_t table[12] = {           // [clone ? 8 + 2 VAL : 4 KLP + 2 VCLIP] + (A == 2)
        ppo_head_loss_kernel<PF_MAX_ACT>, ppo_head_loss_kernel<2>, ppo_head_loss_vclip_kernel<PF_MAX_ACT>, ppo_head_loss_vclip_kernel<2>,
        ppo_head_loss_kl_kernel<PF_MAX_ACT>, ppo_head_loss_kl_kernel<2>, ppo_head_loss_kl_vclip_kernel<PF_MAX_ACT>, ppo_head_loss_kl_vclip_kernel<2>,
        ppo_head_clone_kernel<PF_MAX_ACT, false>, ppo_head_clone_kernel<2, false>, ppo_head_clone_kernel<PF_MAX_ACT, true>, ppo_head_clone_kernel<2, true>};
    const int variant = q.clone ? 8 + 2 * (q.returns != nullptr) : 4 * (q.kl_on != 0) + 2 * (q.v_old != nullptr);
    return table[variant + (q.A == 2)];
}

// the whole minibatch step; fuse_adam = 0: gradients to q.grads instead of the in-place optimiser update.  x3: the GEMM stages (layers 1-2, the layer-1 input
// gradient, the weight gradients) in their split-bf16 instantiations; the head / loss kernel, the flat Adam and the slab sums are the same launches in both modes
int mi_ppo_fused_step(hipStream_t st, PpoFusedParams& q, int fuse_adam, bool x3) {
    { const int rc0 = pf_check_shape(q, "ppo fused step"); if (rc0 != MI_OK) return rc0; }         // before the first launch
    if (fuse_adam && q.M > 256) return mi_fail(MI_ERR_ARG, "ppo fused step: the in-kernel Adam update needs the whole minibatch in one wave (M <= 256)");
    if (q.kl_on && (!q.kl_partial || (q.logp_old != nullptr) != (q.mean_old != nullptr)))
        return mi_fail(MI_ERR_ARG, "ppo fused step: the KL penalty needs its partial buffer, and logp_old / mean_old both or neither");
    if (q.n_wnets != 1 && q.n_wnets != 2) return mi_fail(MI_ERR_ARG, "ppo fused step: n_wnets is 2, or 1 for the policy-only clone step");
    if (q.n_wnets == 1 && !(q.clone && !q.returns)) return mi_fail(MI_ERR_ARG, "ppo fused step: only the clone step without returns leaves the value net out");
    if (q.m_ppo && (q.clone || q.m_ppo < 1 || q.m_ppo >= q.M || !q.demo_states || !q.demo_actions || !q.demo_partial || !q.demo_out || !q.s_gath ||
                    (q.demo_row_idx && q.n_demo_rows < 1) || (q.demo_kind != 0 && q.demo_kind != 1)))
        return mi_fail(MI_ERR_ARG, "ppo fused step: the demonstration term needs PPO rows and demonstration rows, both demonstration tables, its buffers and a kind of 0 / 1");
    q.n_loss_blocks = (q.M + 31) / 32;
    // the demonstration step: one staging launch gathers the M = m_ppo + M_demo state rows of the two tables; every launch but the head kernel then reads them as a
    // contiguous minibatch (the layer-1 kernels are the code and the launches of the other entries), the head kernel keeps both row lists for its scalar gathers
    PpoFusedParams qh = q;
    if (q.m_ppo) {
        const long long n = (long long)q.M * q.din;
        hipLaunchKernelGGL(ppo_demo_stage_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, q.states, q.row_idx, q.n_rows, q.m_ppo,
                           q.demo_states, q.demo_row_idx, q.n_demo_rows, q.M, q.din, q.s_gath);
        q.states = q.s_gath; q.row_idx = nullptr;
    }
    int rc = mi_ppo_fused_trunks(st, q, x3);
    if (rc != MI_OK) return rc;
    rc = ppo_pad(st, q.losses);
    if (rc != MI_OK) return rc;
    hipLaunchKernelGGL(pf_step_head_kernel(qh), dim3(q.n_loss_blocks), dim3(256), 0, st, qh);
    if (x3) hipLaunchKernelGGL(ppo_dh1_kernel<true>, dim3((q.H1 + 31) / 32, q.n_wnets, (q.M + 31) / 32), dim3(256), 0, st, q);
    else hipLaunchKernelGGL(ppo_dh1_kernel<false>, dim3((q.H1 + 31) / 32, q.n_wnets, (q.M + 31) / 32), dim3(256), 0, st, q);
    rc = ppo_pad(st, q.losses);
    if (rc != MI_OK) return rc;
    const int nt1 = (q.H1 + 31) / 32, nt2 = (q.H2 + 31) / 32, kt1 = (q.kin + 31) / 32;
    const int tiles = q.n_wnets * (nt1 * nt2 + kt1 * nt1 + nt2) + 1;         // + the wave that finalises the loss scalars
    q.m_chunk = 0;
    if (fuse_adam) {
        if (x3) hipLaunchKernelGGL((ppo_wgrad_kernel<true, true>), dim3((tiles + 3) / 4), dim3(256), 0, st, q);
        else hipLaunchKernelGGL((ppo_wgrad_kernel<true, false>), dim3((tiles + 3) / 4), dim3(256), 0, st, q);
    } else if (q.M > 256) {                               // row chunks of 256: every chunk stores its own gradient slab, one ordered pass adds them (no atomics: round 4)
        const int chunks = (q.M + 255) / 256;
        if (!q.gslab) return mi_fail(MI_ERR_STATE, "ppo fused step: the engine's workspace has no gradient slabs for minibatches above 256 rows");
        q.m_chunk = 256;
        // (the alignment gaps between the tensors are written by nobody: zeroed, so that the sum leaves zeros there like the memset of the gradient buffer did)
        if (hipMemsetAsync(q.gslab, 0, (size_t)chunks * q.gslab_stride * 4, st) != hipSuccess) return mi_fail(MI_ERR_LAUNCH, "ppo fused step: memset failed");
        if (x3) hipLaunchKernelGGL((ppo_wgrad_kernel<false, true>), dim3((tiles + 3) / 4, chunks), dim3(256), 0, st, q);
        else hipLaunchKernelGGL((ppo_wgrad_kernel<false, false>), dim3((tiles + 3) / 4, chunks), dim3(256), 0, st, q);
        const int rc2 = mi_check_launch("ppo_fused_step");
        if (rc2 != MI_OK) return rc2;
        return mi_reduce_slabs(st, q.gslab, q.gslab_stride, chunks, q.n_params, q.grads, 1);
    } else {
        // policy only: nobody writes the value net's range of the gradient buffer (variables 7..12 lie behind 0..6): it is cleared, so that it reads exactly 0.0
        if (q.n_wnets == 1 && hipMemsetAsync(q.grads + q.off[7], 0, (size_t)(q.n_params - q.off[7]) * 4, st) != hipSuccess)
            return mi_fail(MI_ERR_LAUNCH, "ppo fused step: memset failed");
        if (x3) hipLaunchKernelGGL((ppo_wgrad_kernel<false, true>), dim3((tiles + 3) / 4), dim3(256), 0, st, q);
        else hipLaunchKernelGGL((ppo_wgrad_kernel<false, false>), dim3((tiles + 3) / 4), dim3(256), 0, st, q);
    }
    return mi_check_launch("ppo_fused_step");
}
