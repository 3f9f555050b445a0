// rollout_mlp.hip — layer 1 of the MlpVAE encoder for the rollout step (mi_mlp_rollout_step_batch), straight from the camera bytes of n environments:
//     raw1[e][j] = sum_k (frame[e][k] / 255) W1[k][j]          frames uint8 [n][S] (HBM or pinned host memory), W1 the fp32 master kernel [S][N1] (TF layout)
// Exact fp32 (v_mfma_f32_32x32x2_f32), the byte -> float conversion is u8_to_unit_exact of common.hpp; bias and ReLU are left to the next layer's loader, as
// everywhere in rollout.hip, whose flat layers (mi_rollout_conv_batch, modes 1 / 2) run everything behind this one.
//
// At the reference shape the layer is 38400 x 512: 78.6 MB of weights against 38 KB of input per environment -- below ~32 environments a weight-streaming kernel.
// The grid is ceil(S / KS) blocks and NOTHING else: block b owns k in [KS b, KS b + KS) for every column and every environment (KS = 64, 128 or 256: mlp1_slab).
//   * W1 is streamed once per call.  A wave holds KS k x CT column tiles of weights in 128 registers (KS x CT = 256) -- of a pass, the tiles t0 + w, t0 + 4 + w, ..
//     (32 columns each; a pass is 4 waves x CT tiles) -- and walks ALL row tiles with them (rows = environments, 32 per tile): a weight is loaded by one lane of
//     one wave of one block, once.  N1 past a pass (512 / 256 / 128 columns for KS = 64 / 128 / 256) takes further passes over the same block's k: other
//     columns, so still every weight once.
//   * Every frame byte is fetched by one block only, once: the block first stages its KS bytes of every environment in LDS (KS x ceil32(n) bytes, at most 64 KB) and
//     all four waves and all passes read the A operand from there.  With io = "pinned" that is the one trip of each byte over the host link.
// The K split meets in the raw-sum buffer by fp32 atomics (the choice of rollout.hip; the order of the ceil(S / KS) adds per element is not fixed, two calls can
// differ in the last bits).  The sums must start at zero: rollout_mlp_clear_kernel, launched in front by the same call, clears raw1 and the raw-sum buffers of every
// layer behind it, so a call never depends on what the scratch held on entry.
// Buffer descriptors sized to the operand, no per-lane guards: rows >= n read 0 and their sums fall outside the output descriptor, k >= S reads weights of 0.0.
#include <stdlib.h>
#include "common.hpp"
#include "mi_internal.hpp"
#include "mi355_carla.h"
#include "ppo_fused.hpp"

namespace mi {

typedef float f32x16_m __attribute__((ext_vector_type(16)));

#define MLP1_RSRC(ptr, bytes) __builtin_amdgcn_make_buffer_rsrc((void*)(ptr), 0, (int)(bytes), 0x00020000)
#define MLP1_OOB 0x40000000u                              // a byte offset past every descriptor of this file

constexpr int MLP1_WREGS = 256;                           // k x column tiles a wave holds per pass: KS x CT = 256 (128 registers of weights), whatever the slab

struct RollMlp1Params {
    const unsigned char* frames; const float* w; float* out;     // [n][S] bytes, [S][N] floats, raw sums [n][N] (zeroed; fp32 atomics)
    int S, N, n, row_tiles;                                      // row_tiles = ceil(n / 32)
    unsigned f_bytes, w_bytes, out_bytes;                        // descriptor extents
};

// the raw-sum buffers of one call: the scratch (raw1 | hidden layers | raw means, one piece) and the trunks' raw sums in the PPO engine
__global__ __launch_bounds__(256) void rollout_mlp_clear_kernel(const MiZeroList z) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x, nt = (long long)gridDim.x * 256;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        float* zp = z.p[r]; const long long zn = z.n[r];
        if (!zp) continue;
        if ((((uintptr_t)zp) & 15) == 0) {
            const long long n4 = zn >> 2;
            for (long long i = t; i < n4; i += nt) ((f32x4*)zp)[i] = f32x4{0.f, 0.f, 0.f, 0.f};
            for (long long i = (n4 << 2) + t; i < zn; i += nt) zp[i] = 0.f;
        } else {
            for (long long i = t; i < zn; i += nt) zp[i] = 0.f;
        }
    }
}

// the fragments of the wave's CT = 256 / KS column tiles of pass t0: b[c][u][e] = W1[k0 + 8 u + 4 lgrp + e][32 (t0 + 4 c + wave) + lrow]
// (a column past N1 reads its neighbour in the next weight row, or 0.0 behind the matrix; its sums are dropped on output.  k >= S lies behind the matrix: 0.0)
template <int KS>
__device__ __forceinline__ void mlp1_load_w(const RollMlp1Params& p, const __amdgpu_buffer_rsrc_t rsW, unsigned k0, int t0, int ntile, int wave, int lrow, int lgrp, f32x4 (*b)[KS / 8]) {
    const unsigned ldw = (unsigned)p.N;
#pragma unroll
    for (int c = 0; c < MLP1_WREGS / KS; ++c) {
        const int tile = t0 + 4 * c + wave;
        if (tile >= ntile) continue;                          // (wave-uniform)
        const unsigned ncol = (unsigned)(tile * 32 + lrow);
#pragma unroll
        for (int u = 0; u < KS / 8; ++u) {
            const unsigned wo = ((k0 + (unsigned)(u * 8 + lgrp * 4)) * ldw + ncol) * 4u;
#pragma unroll
            for (int e = 0; e < 4; ++e) b[c][u][e] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsW, (int)(wo + (unsigned)e * ldw * 4u), 0, 0));
        }
    }
}

template <int KS>
__global__ __launch_bounds__(256) void rollout_mlp_layer1_kernel(const RollMlp1Params p) {
    // the block's KS bytes of every row: dword d (bytes 4 d .. 4 d + 3 of the slab) of row r at r * DW + (d ^ (r & (DW - 1))), DW = KS / 4
    constexpr int CT = MLP1_WREGS / KS, NU = KS / 8, DW = KS / 4;
    extern __shared__ unsigned mlp1_lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lrow = lane & 31, lgrp = lane >> 5;
    const unsigned k0 = blockIdx.x * (unsigned)KS;
    const __amdgpu_buffer_rsrc_t rsF = MLP1_RSRC(p.frames, p.f_bytes);
    const __amdgpu_buffer_rsrc_t rsW = MLP1_RSRC(p.w, p.w_bytes);
    const __amdgpu_buffer_rsrc_t rsO = MLP1_RSRC(p.out, p.out_bytes);
    const int ntile = (p.N + 31) >> 5;
    f32x4 b[CT][NU];
    mlp1_load_w<KS>(p, rsW, k0, 0, ntile, wave, lrow, lgrp, b);          // in flight under the staging below
    const int ndw = p.row_tiles * 32 * DW;
    for (int i = tid; i < ndw; i += 256) {
        const int r = i / DW, d = i & (DW - 1);
        const unsigned k = k0 + 4u * (unsigned)d;
        // a row past n lies behind the descriptor (0); behind the last byte of a row lies the next row, so k >= S is sent there explicitly
        const unsigned off = k < (unsigned)p.S ? (unsigned)r * (unsigned)p.S + k : MLP1_OOB;
        mlp1_lds[r * DW + (d ^ (r & (DW - 1)))] = (unsigned)__builtin_amdgcn_raw_buffer_load_b32(rsF, (int)off, 0, 0);
    }
    __syncthreads();
    const unsigned rowb = (unsigned)p.N * 4u;
    for (int t0 = 0;;) {
        for (int rt = 0; rt < p.row_tiles; ++rt) {
            const int r = rt * 32 + lrow;
            f32x4 a[NU];
#pragma unroll
            for (int u = 0; u < NU; ++u) {
                const unsigned v = mlp1_lds[r * DW + ((u * 2 + lgrp) ^ (r & (DW - 1)))];
#pragma unroll
                for (int e = 0; e < 4; ++e) a[u][e] = u8_to_unit_exact((float)((v >> (8 * e)) & 255u));
            }
#pragma unroll
            for (int c = 0; c < CT; ++c) {
                const int tile = t0 + 4 * c + wave;
                if (tile >= ntile) continue;                  // (wave-uniform)
                f32x16_m acc;
#pragma unroll
                for (int q = 0; q < 16; ++q) acc[q] = 0.f;
#pragma unroll
                for (int u = 0; u < NU; ++u)
#pragma unroll
                    for (int s = 0; s < 4; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u][s], b[c][u][s], acc, 0, 0, 0);
                const unsigned ncol = (unsigned)(tile * 32 + lrow);
                const unsigned col = ncol < (unsigned)p.N ? ncol * 4u : MLP1_OOB;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    if (rt * 32 + 8 * q >= p.n) continue;     // (wave-uniform: the 8 rows of this group all lie past n)
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const unsigned mm = (unsigned)(rt * 32 + e + 8 * q + 4 * lgrp);
                        __builtin_amdgcn_raw_ptr_buffer_atomic_fadd_f32(acc[4 * q + e], rsO, (int)(mm * rowb + col), 0, 0);     // rows past n fall outside the descriptor
                    }
                }
            }
        }
        t0 += 4 * CT;
        if (t0 >= ntile) break;
        mlp1_load_w<KS>(p, rsW, k0, t0, ntile, wave, lrow, lgrp, b);
    }
}

}  // namespace mi

using namespace mi;

// the K-slab of a call.  One row tile (n <= 32): 64, the most blocks in flight under the weight stream (measured: 83.6 / 88.1 us per call at 1 / 8 environments
// against 85.0 / 92.2 with 256).  More row tiles: the adds onto raw1 are what grows, and a wider slab means fewer of them per element: the widest of 256 / 128 / 64
// whose stage of ceil32(n) rows fits 64 KB of LDS, n <= 256 / <= 512 / any n (64 environments: 211 / 228 / 263 us per call with 256 / 128 / 64).
static int mlp1_slab(int n) {
    const int rows = (n + 31) / 32 * 32;
    return rows <= 32 ? 64 : rows * 256 <= 65536 ? 256 : rows * 128 <= 65536 ? 128 : 64;
}

// clears `zero` (the raw-sum buffers of the whole call; raw1 among them) and adds layer 1 of n environments onto raw1 [n][N1].  frames 4-byte aligned.
int mi_rollout_mlp_layer1(hipStream_t st, const unsigned char* frames, const float* w1, float* raw1, int S, int N1, int n, const MiZeroList* zero) {
    if (S < 4 || (S & 3) || N1 < 1) return mi_fail(MI_ERR_SHAPE, "rollout mlp layer 1: the frame size must be a multiple of 4");
    if (n < 1 || n > MI_ROLLOUT_MAX_ENVS) return mi_fail(MI_ERR_ARG, "rollout mlp layer 1: 1 <= n <= MI_ROLLOUT_MAX_ENVS");
    const long long fb = (long long)n * S, wb = (long long)S * N1 * 4, ob = (long long)n * N1 * 4, rows = (n + 31) / 32 * 32;
    // (the offsets the kernel forms run over the padded tiles: rows up to the row tile, k up to the slab, columns up to the column tile)
    if (rows * S >= 0x40000000ll || ((long long)S + 256) * ((long long)N1 + 32) * 4 >= 0x40000000ll || rows * ((long long)N1 + 32) * 4 >= 0x40000000ll)
        return mi_fail(MI_ERR_SHAPE, "rollout mlp layer 1: operand beyond 1 GiB");
    RollMlp1Params p = {};
    p.frames = frames; p.w = w1; p.out = raw1; p.S = S; p.N = N1; p.n = n; p.row_tiles = (n + 31) / 32;
    p.f_bytes = (unsigned)fb; p.w_bytes = (unsigned)wb; p.out_bytes = (unsigned)ob;
    MiZeroList z = {};
    if (zero) z = *zero;
    long long zf = 0;
    for (int r = 0; r < 3; ++r) zf += z.p[r] ? z.n[r] : 0;
    long long zb = (zf / 4 + 255) / 256;
    if (zb < 1) zb = 1;
    if (zb > 512) zb = 512;
    hipLaunchKernelGGL(rollout_mlp_clear_kernel, dim3((unsigned)zb), dim3(256), 0, st, z);
    const int ks = mlp1_slab(n);
    const dim3 g((unsigned)((S + ks - 1) / ks));
    const size_t lds = (size_t)rows * ks;
    if (ks == 256) hipLaunchKernelGGL(rollout_mlp_layer1_kernel<256>, g, dim3(256), lds, st, p);
    else if (ks == 128) hipLaunchKernelGGL(rollout_mlp_layer1_kernel<128>, g, dim3(256), lds, st, p);
    else hipLaunchKernelGGL(rollout_mlp_layer1_kernel<64>, g, dim3(256), lds, st, p);
    return mi_check_launch("rollout_mlp_layer1_kernel");
}
