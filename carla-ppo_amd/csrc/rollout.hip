// rollout.hip — the inference path of the rollout loop (B = 1, and n environments per call: the *_batch kernels) as ONE C-ABI call: raw uint8 camera frame + measurements ->
// ConvVAE encoder mean z (vae/models.py:199-202, 249-256) -> state = [z, measurements] (vae_common.py:45-59) -> policy / value heads
// (ppo.py:231-251) -> (action, value, z) in one buffer (device memory or pinned host memory).  Exact fp32 (v_mfma_f32_32x32x2_f32).
//
// At one frame every layer is a tiny GEMM with a long K (conv4: 24 x 256 x 2048; the trunks: 1 x 500 x 67, 1 x 300 x 500): the training
// kernels give such a shape a handful of blocks that walk K serially (10-70 us each).  Here every layer is split over K as well: a wave owns
// a (32 rows x 32 columns x 64 k) unit, the four waves of a block meet in LDS and add their tile to the zeroed raw output with fp32 atomics;
// bias + ReLU of a layer are applied by the NEXT layer's operand loader, so no layer needs a finishing pass, and the step is a chain of
// eight launches whose cost is their latency, not their work:
//     conv1 (also clears the raw buffers) -> conv2 -> conv3 -> conv4 -> mean -> trunk layer 1 (both nets) -> trunk layer 2 (both nets) -> heads
#include <stdio.h>
#include <stdlib.h>
#include <type_traits>
#include "common.hpp"
#include "mi_internal.hpp"
#include "mi355_carla.h"
#include "ppo_fused.hpp"

namespace mi {

typedef float f32x16_r __attribute__((ext_vector_type(16)));

// Every operand goes through a buffer descriptor whose extent is the operand's size: rows past M are clamped (their results are dropped by the
// output descriptor), k past K and columns past the matrix read 0.0 from the hardware range check -- no per-lane branches, so the kernels are
// a few hundred instructions long; at one wave per SIMD the instruction count IS the kernel time (the first form, with a guard around every
// load, was 3,500 instructions and 6-7 us per layer).
struct RollConvParams {
    const float* x; const float* x_bias;                 // input [IH,IW,C]; x_bias != NULL: raw sums of the previous layer: x + x_bias[c] on load, then ReLU if `relu`
    const float* x_tail; int split;                       // state-vector form (vec = 0): elements k >= split come from x_tail[k - split] as they are (the measurements)
    const float* w; int ldw;                              // weights [K][ldw] (TF HWIO flattened: k = (kh KW + kw) C + ci), N <= ldw columns used
    float* out;                                           // raw output [M][N] (zeroed; fp32 atomics)
    long long x_net, xb_net, w_net, out_net;              // flat only: blockIdx.y = net (policy / value trunk): per-net strides in floats
    unsigned x_bytes, xb_bytes, tail_bytes, w_bytes, out_bytes;   // descriptor extents
    int IW, C, OW, M, N, K, KW, flat, relu, c_shift, vec; // flat = 1: x is a vector of K values, M = 1; c_shift = log2(C) or -1
};

// The batched step (n environments in one call) carries the same fields plus the row geometry: rows run over n * OH * OW output pixels (conv) or
// over the n environments (flat layers); the image / environment index is taken from the row.  A type of its own, so the B = 1 instantiations
// see the parameter block (and compile to the code) they always had.
struct RollConvBatchParams : RollConvParams {
    int OHW; unsigned img_stride;                         // conv: output pixels per image; floats between two images of x
    int row_tiles; unsigned x_row, t_row;                 // flat: blockIdx.y = net * row_tiles + row tile; floats between two rows of x / of x_tail
};

#define ROLL_RSRC(ptr, bytes) __builtin_amdgcn_make_buffer_rsrc((void*)(ptr), 0, (int)(bytes), 0x00020000)
#define ROLL_OOB 0x40000000u                              // a byte offset past every descriptor of this file

__device__ __forceinline__ float roll_ld(const __amdgpu_buffer_rsrc_t r, unsigned byte_off) { return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, (int)byte_off, 0, 0)); }
__device__ __forceinline__ f32x4 roll_ld4(const __amdgpu_buffer_rsrc_t r, unsigned byte_off) { return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r, (int)byte_off, 0, 0)); }

// one block unit (bx, by, bz) of the grid (ceil(N / 32), ceil(M / 32) | nets, ceil(K / 256)); wave w of the block: k in [256 bz + 64 w, + 64)
// MODE: 0 = conv, power-of-two C and KW = 4 (shifts); 1 = flattened input, power-of-two C (the mean head); 2 = flattened, bias indexed by k
// (trunk layer 2); 3 = the assembled state vector (trunk layer 1); 4 = conv, any C / KW
// P = RollConvBatchParams: the batched form.  conv: M = n OH OW rows, the lane's row m lies in image m / OHW.  flat: M = n rows, one per environment, so the
// MFMA's 32 rows carry 32 environments instead of one; grid.y = nets x row tiles; row m of x / x_tail starts at m x_row / m t_row.  A load of k >= K is sent
// past the descriptor explicitly (behind the last k of a row lies the next row); rows past M stay clamped on load and dropped by the output descriptor.
template <int MODE, class P>
__device__ __forceinline__ void roll_conv_unit(const P& p, int bx, int by, int bz, f32x4 (*red)[4][64]) {
    constexpr bool FLAT = MODE == 1 || MODE == 2 || MODE == 3;
    constexpr bool NB = std::is_same<P, RollConvBatchParams>::value;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lrow = lane & 31, lgrp = lane >> 5;
    int net = FLAT ? by : 0, m0 = FLAT ? 0 : by * 32;
    if constexpr (NB && FLAT) { net = by / p.row_tiles; m0 = (by - net * p.row_tiles) * 32; }
    const int n0 = bx * 32, kb = bz * 256 + wave * 64;
    const int n = n0 + lrow, m = min(m0 + lrow, p.M - 1);
    const __amdgpu_buffer_rsrc_t rsX = ROLL_RSRC(p.x + net * p.x_net, p.x_bytes);
    const __amdgpu_buffer_rsrc_t rsB = ROLL_RSRC(p.x_bias ? p.x_bias + net * p.xb_net : p.x, p.xb_bytes);
    const __amdgpu_buffer_rsrc_t rsT = ROLL_RSRC(p.x_tail ? p.x_tail : p.x, p.tail_bytes);
    const __amdgpu_buffer_rsrc_t rsW = ROLL_RSRC(p.w + net * p.w_net, p.w_bytes);
    int mi = m; unsigned xrow = 0u, trow = 0u;            // batched: where this lane's image / row starts in x and in x_tail (floats)
    if constexpr (NB && !FLAT) { const int img = m / p.OHW; mi = m - img * p.OHW; xrow = (unsigned)img * p.img_stride; }
    if constexpr (NB && FLAT) { xrow = (unsigned)m * p.x_row; trow = (unsigned)m * p.t_row; }
    const int oy = FLAT ? 0 : mi / p.OW, ox = mi - oy * p.OW;
    const unsigned pix = FLAT ? 0u : xrow + (unsigned)((2 * oy * p.IW + 2 * ox) * p.C);
    const unsigned ldw = (unsigned)p.ldw;
    f32x4 a[8], b[8], bi[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        const int k = kb + u * 8 + lgrp * 4;               // 4 consecutive k: one (kh, kw), 4 consecutive input channels (C % 4 == 0)
        if (MODE != 3) {
            unsigned off, ci;
            if (FLAT) {
                off = (unsigned)k; ci = MODE == 1 ? (unsigned)(k & (p.C - 1)) : (unsigned)k;
                if constexpr (NB) off = k < p.K ? xrow + (unsigned)k : (ROLL_OOB >> 2);
            }
            else {
                int tap, kh, kw;
                if (MODE == 0) { tap = k >> p.c_shift; ci = (unsigned)(k & (p.C - 1)); kh = tap >> 2; kw = tap & 3; }
                else { tap = k / p.C; ci = (unsigned)(k - tap * p.C); kh = tap / p.KW; kw = tap - kh * p.KW; }
                off = k < p.K ? pix + (unsigned)((kh * p.IW + kw) * p.C) + ci : (ROLL_OOB >> 2);
            }
            a[u] = roll_ld4(rsX, off * 4u);
            bi[u] = roll_ld4(rsB, ci * 4u);
        } else {                                           // the assembled state vector [x + bias | tail], any K: x / bias descriptors end at `split`
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const unsigned ke = (unsigned)(k + e);
                if constexpr (NB) {
                    const unsigned xo = ke < (unsigned)p.split ? (xrow + ke) * 4u : ROLL_OOB;
                    const unsigned to = (ke >= (unsigned)p.split && ke < (unsigned)p.K) ? (trow + ke - (unsigned)p.split) * 4u : ROLL_OOB;
                    a[u][e] = roll_ld(rsX, xo) + roll_ld(rsT, to);
                } else {
                    a[u][e] = roll_ld(rsX, ke * 4u) + roll_ld(rsT, (ke - (unsigned)p.split) * 4u);
                }
                bi[u][e] = roll_ld(rsB, ke * 4u);
            }
        }
        const unsigned wo = ((unsigned)k * ldw + (unsigned)n) * 4u;
#pragma unroll
        for (int e = 0; e < 4; ++e) b[u][e] = roll_ld(rsW, wo + (unsigned)e * ldw * 4u);
    }
    f32x16_r acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    const float floor_v = p.relu ? 0.f : -__builtin_inff();
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        f32x4 av;
#pragma unroll
        for (int e = 0; e < 4; ++e) av[e] = fmaxf(a[u][e] + bi[u][e], floor_v);
#pragma unroll
        for (int s = 0; s < 4; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[s], b[u][s], acc, 0, 0, 0);
    }
    if (wave > 0) {
#pragma unroll
        for (int q = 0; q < 4; ++q) red[wave - 1][q][lane] = f32x4{acc[4 * q], acc[4 * q + 1], acc[4 * q + 2], acc[4 * q + 3]};
    }
    __syncthreads();
    if (wave == 0) {
        const __amdgpu_buffer_rsrc_t rsO = ROLL_RSRC(p.out + net * p.out_net, p.out_bytes);
        const unsigned col = n < p.N ? (unsigned)n * 4u : ROLL_OOB, rowb = (unsigned)p.N * 4u;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const f32x4 r0 = red[0][q][lane], r1 = red[1][q][lane], r2 = red[2][q][lane];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float v = ((acc[4 * q + e] + r0[e]) + (r1[e] + r2[e]));
                const unsigned mm = (unsigned)(m0 + e + 8 * q + 4 * lgrp);
                __builtin_amdgcn_raw_ptr_buffer_atomic_fadd_f32(v, rsO, (int)(mm * rowb + col), 0, 0);     // rows past M fall outside the descriptor
            }
        }
    }
}

template <int MODE>
__global__ __launch_bounds__(256) void rollout_conv_kernel(const RollConvParams p) {
    __shared__ f32x4 red[3][4][64];
    roll_conv_unit<MODE>(p, blockIdx.x, blockIdx.y, blockIdx.z, red);
}

template <int MODE>
__global__ __launch_bounds__(256) void rollout_conv_batch_kernel(const RollConvBatchParams p) {
    __shared__ f32x4 red[3][4][64];
    roll_conv_unit<MODE>(p, blockIdx.x, blockIdx.y, blockIdx.z, red);
}

static int conv_mode(const RollConvParams& p) { return !p.flat ? ((p.c_shift >= 0 && p.KW == 4) ? 0 : 4) : (!p.vec ? 3 : (p.c_shift >= 0 ? 1 : 2)); }

static void launch_conv_batch(hipStream_t st, const dim3& g, const RollConvBatchParams& p) {
    switch (conv_mode(p)) {
        case 0: hipLaunchKernelGGL(rollout_conv_batch_kernel<0>, g, dim3(256), 0, st, p); break;
        case 1: hipLaunchKernelGGL(rollout_conv_batch_kernel<1>, g, dim3(256), 0, st, p); break;
        case 2: hipLaunchKernelGGL(rollout_conv_batch_kernel<2>, g, dim3(256), 0, st, p); break;
        case 3: hipLaunchKernelGGL(rollout_conv_batch_kernel<3>, g, dim3(256), 0, st, p); break;
        default: hipLaunchKernelGGL(rollout_conv_batch_kernel<4>, g, dim3(256), 0, st, p); break;
    }
}

static void launch_conv(hipStream_t st, const dim3& g, const RollConvParams& p) {
    const int mode = conv_mode(p);
    switch (mode) {
        case 0: hipLaunchKernelGGL(rollout_conv_kernel<0>, g, dim3(256), 0, st, p); break;
        case 1: hipLaunchKernelGGL(rollout_conv_kernel<1>, g, dim3(256), 0, st, p); break;
        case 2: hipLaunchKernelGGL(rollout_conv_kernel<2>, g, dim3(256), 0, st, p); break;
        case 3: hipLaunchKernelGGL(rollout_conv_kernel<3>, g, dim3(256), 0, st, p); break;
        default: hipLaunchKernelGGL(rollout_conv_kernel<4>, g, dim3(256), 0, st, p); break;
    }
}

// conv1 from the raw uint8 frame: out[m, n] = relu(sum_k (frame[..] / 255) W[k, n] + b[n]), K = KH KW 3 = 48; one wave per 32 pixels x 32 channels.
// The byte -> float32(k) / float32(255) conversion is the exact in-register form of common.hpp.  grid ceil(M / 128) blocks of 4 waves.
// ROW = KW * Cs when that is 12 (the reference's 4 x 4 x RGB kernel): a patch row is 12 contiguous bytes, 4 consecutive k never straddle two
// rows and the byte address is even, so a lane fetches its 4 patch values as two 16-bit loads; ROW = 0: any shape, one byte load per value.
// The launch also clears the raw-sum buffers of the layers behind it.
struct RollConv1Params {
    const unsigned char* frame; const float* w; const float* bias; float* out;
    int IH, IW, Cs, OW, M, N, KW, K;
    MiZeroList z;
};

struct RollConv1BatchParams : RollConv1Params { int OHW; unsigned frame_stride; };     // batched: M = n OHW pixels, frame e starts frame_stride bytes behind frame e - 1

__device__ __forceinline__ void roll_zero(const MiZeroList& z, long long t, long long nt) {
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

// 32 pixels x 32 channels of conv1 by one wave; wunit = index of the 32-pixel group.  Same descriptor discipline as roll_conv_unit.
template <int ROW, class P>
__device__ __forceinline__ void roll_conv1_unit(const P& c, int wunit) {
    constexpr bool NB = std::is_same<P, RollConv1BatchParams>::value;
    const int IW = c.IW, Cs = c.Cs, OW = c.OW, M = c.M, N = c.N, KW = c.KW, K = c.K;
    const int lane = threadIdx.x & 63, lrow = lane & 31, lgrp = lane >> 5;
    const int m0 = wunit * 32;
    if (m0 >= M) return;
    const int m = min(m0 + lrow, M - 1), n = lrow;
    unsigned f_bytes = (unsigned)(c.IH * IW * Cs), f_off = 0u; int mi = m;
    if constexpr (NB) { const int img = m / c.OHW; mi = m - img * c.OHW; f_off = (unsigned)img * c.frame_stride; f_bytes = (unsigned)(M / c.OHW) * c.frame_stride; }
    const __amdgpu_buffer_rsrc_t rsF = ROLL_RSRC(c.frame, f_bytes);
    const __amdgpu_buffer_rsrc_t rsW = ROLL_RSRC(c.w, K * N * 4);
    const __amdgpu_buffer_rsrc_t rsO = ROLL_RSRC(c.out, M * N * 4);
    const int oy = mi / OW, ox = mi - oy * OW;
    f32x16_r acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    f32x4 a[6], b[6];
    const unsigned base = f_off + (unsigned)((2 * oy * IW + 2 * ox) * Cs), rowbytes = (unsigned)(IW * Cs);
#pragma unroll
    for (int u = 0; u < 6; ++u) {
        const int k0 = u * 8 + lgrp * 4;
        if (ROW == 12) {
            const int kh = k0 / 12, kr = k0 - kh * 12;
            const unsigned o = base + (unsigned)kh * rowbytes + (unsigned)kr;
            const unsigned v = (unsigned)__builtin_amdgcn_raw_buffer_load_b16(rsF, (int)o, 0, 0) | ((unsigned)__builtin_amdgcn_raw_buffer_load_b16(rsF, (int)o + 2, 0, 0) << 16);
#pragma unroll
            for (int e = 0; e < 4; ++e) a[u][e] = u8_to_unit_exact((float)((v >> (8 * e)) & 255u));
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int k = k0 + e;
                const int tap = k / Cs, ci = k - tap * Cs, kh = tap / KW, kw = tap - kh * KW;
                a[u][e] = u8_to_unit_exact((float)__builtin_amdgcn_raw_buffer_load_b8(rsF, k < K ? (int)(base + (unsigned)kh * rowbytes + (unsigned)(kw * Cs + ci)) : (int)ROLL_OOB, 0, 0));
            }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) b[u][e] = roll_ld(rsW, (unsigned)((k0 + e) * N + n) * 4u);      // k >= K: past the descriptor, 0.0
    }
#pragma unroll
    for (int u = 0; u < 6; ++u)
#pragma unroll
        for (int s = 0; s < 4; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u][s], b[u][s], acc, 0, 0, 0);
    const float bn = roll_ld(ROLL_RSRC(c.bias, N * 4), (unsigned)n * 4u);
    const unsigned col = n < N ? (unsigned)n * 4u : ROLL_OOB, rowb = (unsigned)N * 4u;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const unsigned mm = (unsigned)(m0 + (r & 3) + 8 * (r >> 2) + 4 * lgrp);
        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, fmaxf(acc[r] + bn, 0.f)), rsO, (int)(mm * rowb + col), 0, 0);
    }
}

template <int ROW>
__global__ __launch_bounds__(256) void rollout_conv1_kernel(const RollConv1Params c) {
    roll_zero(c.z, (long long)blockIdx.x * 256 + threadIdx.x, (long long)gridDim.x * 256);
    roll_conv1_unit<ROW>(c, blockIdx.x * 4 + (threadIdx.x >> 6));
}

template <int ROW>
__global__ __launch_bounds__(256) void rollout_conv1_batch_kernel(const RollConv1BatchParams c) {
    roll_zero(c.z, (long long)blockIdx.x * 256 + threadIdx.x, (long long)gridDim.x * 256);
    roll_conv1_unit<ROW>(c, blockIdx.x * 4 + (threadIdx.x >> 6));
}

// heads of the rollout step: h2 = relu(raw layer-2 sums + bias) of both trunks -> action mean (tanh, scaled to the action range, ppo.py:56-67),
// the sampled / greedy action (ppo.py:81-88, clipped), the value (ppo.py:70-71), and the encoder mean z beside them: out = [action | value | z].
// One block; the arithmetic of the finishing thread is that of ppo_predict_head_kernel.
struct RollHeadParams {
    const float *Wm, *bm, *logstd, *b2p, *b2v, *Wv, *bv, *low, *high;
    const float *h2raw, *mean_raw, *mean_bias, *noise;
    float *mean_out, *out;
    int A, H2, z_dim, greedy;
};

// where the recording heads store a call row besides `out`: row r of the tables (all NULL: this block records nothing)
struct RollRecRow { float *state, *action, *value; };

template <int NA, bool REC = false>
__device__ __forceinline__ void roll_head(const RollHeadParams& q, float (*red)[NA + 1], const int vnet, const RollRecRow rec = RollRecRow{}) {     // vnet: floats from the policy trunk's h2 row to the value trunk's
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, A = q.A, H2 = q.H2;
    float au[NA], av = 0.f;
#pragma unroll
    for (int a = 0; a < NA; ++a) au[a] = 0.f;
    for (int j = tid; j < H2; j += 256) {
        const float hp = fmaxf(q.h2raw[j] + q.b2p[j], 0.f), hv = fmaxf(q.h2raw[vnet + j] + q.b2v[j], 0.f);
        av += hv * q.Wv[j];
#pragma unroll
        for (int a = 0; a < NA; ++a) if (a < A) au[a] += hp * q.Wm[(long long)j * A + a];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        av += __shfl_xor(av, o, 64);
#pragma unroll
        for (int a = 0; a < NA; ++a) au[a] += __shfl_xor(au[a], o, 64);
    }
    if (lane == 0) {
#pragma unroll
        for (int a = 0; a < NA; ++a) red[wave][a] = au[a];
        red[wave][NA] = av;
    }
    float* out = q.out;
    for (int i = tid; i < q.z_dim; i += 256) {
        const float zv = q.mean_raw[i] + q.mean_bias[i];
        out[A + 1 + i] = zv;
        if constexpr (REC) { if (rec.state) rec.state[i] = zv; }
    }
    __syncthreads();
    if (tid > A) return;
    if (tid == A) {
        const float v = ((red[0][NA] + red[1][NA]) + (red[2][NA] + red[3][NA])) + q.bv[0];
        out[A] = v;
        if constexpr (REC) { if (rec.value) rec.value[0] = v; }
        return;
    }
    float u = 0.f;
#pragma unroll
    for (int a = 0; a < NA; ++a) if (a == tid) u = (red[0][a] + red[1][a]) + (red[2][a] + red[3][a]);
    const float lo = q.low[tid], hi = q.high[tid];
    const float mean = lo + ((tanhf(u + q.bm[tid]) + 1.0f) * 0.5f) * (hi - lo);
    if (q.mean_out) q.mean_out[tid] = mean;
    float act = mean;
    if (!q.greedy) act = fminf(fmaxf(mean + expf(q.logstd[tid]) * q.noise[tid], lo), hi);
    out[tid] = act;
    if constexpr (REC) { if (rec.action) rec.action[tid] = act; }
}

template <int NA>
__global__ __launch_bounds__(256) void rollout_head_kernel(const RollHeadParams q) {
    __shared__ float red[4][NA + 1];
    roll_head<NA>(q, red, q.H2);
}

// the batched heads: block e finishes environment e -- row e of both trunks' raw sums ([net][n][H2]), of the raw means and of the noise; output row e
template <int NA>
__global__ __launch_bounds__(256) void rollout_head_batch_kernel(const RollHeadParams q0, const int n) {
    __shared__ float red[4][NA + 1];
    RollHeadParams q = q0;
    const long long e = blockIdx.x;
    q.h2raw += e * q.H2; q.mean_raw += e * q.z_dim; q.out += e * (q.A + 1 + q.z_dim);
    if (q.noise) q.noise += e * q.A;
    if (q.mean_out) q.mean_out += e * q.A;
    roll_head<NA>(q, red, n * q.H2);
}

// the recording heads (mi_rollout_step_batch_rec): rollout_head_batch_kernel's arithmetic, and block e also stores what it computed as row r = table_rows[e] of the
// horizon-batch tables an update trains from: states[r] = [z | measurements[e]], actions[r], values[r] -- the same registers that go to `out`, plain vector stores.
// r outside [0, n_table_rows) (-1 = "do not record this environment") stores nothing into the tables, whatever its value.
struct RollRecParams {
    const int* table_rows; long long n_table_rows;       // [n] (the step's input buffer: HBM or pinned host memory); rows the tables hold
    const float* meas; int n_meas, din;                   // measurements [n][n_meas]; din = z_dim + n_meas floats per states row
    float *states, *actions, *values;
};

template <int NA>
__global__ __launch_bounds__(256) void rollout_head_rec_kernel(const RollHeadParams q0, const int n, const RollRecParams t) {
    __shared__ float red[4][NA + 1];
    RollHeadParams q = q0;
    const long long e = blockIdx.x;
    q.h2raw += e * q.H2; q.mean_raw += e * q.z_dim; q.out += e * (q.A + 1 + q.z_dim);
    if (q.noise) q.noise += e * q.A;
    if (q.mean_out) q.mean_out += e * q.A;
    const long long r = t.table_rows[e];
    RollRecRow rec = {};
    if (r >= 0 && r < t.n_table_rows) {
        rec.action = t.actions + r * q.A; rec.value = t.values + r;
        if (t.states) {                                   // (NULL: the stacked form, whose row rollout_stack_kernel has written)
            rec.state = t.states + r * t.din;
            for (int j = threadIdx.x; j < t.n_meas; j += 256) rec.state[q.z_dim + j] = t.meas[e * t.n_meas + j];
        }
    }
    roll_head<NA, true>(q, red, n * q.H2, rec);
}

// the value-only heads (mi_rollout_value_batch_rec): the value of roll_head for environment e = blockIdx.x -- the same terms in the same order: thread-strided partial
// sums over H2, the wave butterfly, the four waves as (w0 + w1) + (w2 + w3), + bias -- from the VALUE trunk's raw layer-2 sums alone; nothing of the policy net is read.
// The value goes to out[e] and, as a plain vector store, to final_values[table_rows[e]]; a row outside [0, n_table_rows) records nothing.
struct RollValueParams {
    const float *h2raw, *b2v, *Wv, *bv;                   // h2raw: row 0 of the value trunk's raw sums [n][H2]
    int H2;
    const int* table_rows; long long n_table_rows;
    float *out, *final_values;
};

__global__ __launch_bounds__(256) void rollout_value_rec_kernel(const RollValueParams q) {
    __shared__ float red[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, H2 = q.H2;
    const long long e = blockIdx.x;
    const float* h2 = q.h2raw + e * H2;
    float av = 0.f;
    for (int j = tid; j < H2; j += 256) {
        const float hv = fmaxf(h2[j] + q.b2v[j], 0.f);
        av += hv * q.Wv[j];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) av += __shfl_xor(av, o, 64);
    if (lane == 0) red[wave] = av;
    __syncthreads();
    if (tid != 0) return;
    const float v = ((red[0] + red[1]) + (red[2] + red[3])) + q.bv[0];
    q.out[e] = v;
    const long long r = q.table_rows[e];
    if (r >= 0 && r < q.n_table_rows) q.final_values[r] = v;
}

// the observation normaliser (mi_rollout_step_batch_norm / mi_rollout_value_batch_norm), launched between the mean layer and trunk layer 1: block e normalises the
// din entries of environment e's state, thread t the columns t, t + 128, .. (no division anywhere: the kernel is its latency).  s = the raw entry (mean_raw + mean_bias
// for a latent column -- the sum the heads return as z --, the measurement as fed for the others); nstate[e][j] = obs_normalize(s, obs_mean[j], obs_inv_std[j], clip),
// and the same register as a plain vector store to tab_states[table_rows[e]][j] where that row lies in [0, n_table_rows) (table_rows NULL: nothing is recorded).
// Trunk layer 1 then reads nstate as a state vector without bias or tail.
struct RollObsNormParams {
    const float *mean_raw, *mean_bias, *meas;             // raw means [n][z_dim], the mean layer's bias [z_dim], measurements [n][din - z_dim]
    const float *obs_mean, *obs_inv_std; float clip;      // fp32 [din] each; clip > 0 (+inf: never clamps)
    float* nstate;                                        // [n][din]
    const int* table_rows; long long n_table_rows; float* tab_states;
    int n, z_dim, din;
};

__global__ __launch_bounds__(128) void rollout_obs_norm_kernel(const RollObsNormParams p) {
    const long long e = blockIdx.x;
    if (e >= p.n) return;
    const float* z = p.mean_raw + e * p.z_dim;
    const long long ms = e * (p.din - p.z_dim) - p.z_dim;             // measurement j - z_dim of environment e is p.meas[ms + j]
    float* dst = p.nstate + e * p.din;
    float* tab = nullptr;
    if (p.table_rows) {
        const long long r = p.table_rows[e];
        if (r >= 0 && r < p.n_table_rows) tab = p.tab_states + r * p.din;
    }
    for (int j = threadIdx.x; j < p.din; j += 128) {
        const float s = j < p.z_dim ? z[j] + p.mean_bias[j] : p.meas[ms + j];
        const float v = obs_normalize(s, p.obs_mean[j], p.obs_inv_std[j], p.clip);
        dst[j] = v;
        if (tab) tab[j] = v;
    }
}

// latent stacking (mi_rollout_step_batch_stack / mi_rollout_value_batch_stack), launched where the normaliser runs: block e assembles environment e's state
//     [z_t | old_1 | .. | old_{k-1} | measurements],   z_t = mean_raw + mean_bias (the sum the heads return as z),   old_i = first ? z_t : hist[lane][i - 1]
// (a select: what a `first` row's lane holds never reaches the row; a lane outside [0, n_lanes) is `first` and its history is neither read nor written).  Thread t
// holds the columns t, t + 128, .. in registers -- din <= 1024: at most 8 -- and every store is a plain vector store of such a register: the raw row to sstate (with
// obs_mean: obs_normalize of it, the normaliser's formula) and, where table_rows[e] lies in [0, n_table_rows), to tab_states (with obs_mean: the normalised row there,
// the raw one to tab_raw_states); the k - 1 older latents to older[e].  Then a barrier -- every read of the lane's history lies before it -- and with `advance` the
// lane's history becomes the row's first (k - 1) z_dim columns, [z_t | old_1 | .. | old_{k-2}].  Lanes of one call are distinct (the caller's duty): block e alone
// touches hist[lanes[e]].  Trunk layer 1 then reads sstate as a state vector without bias or tail.
struct RollStackParams {
    const float *mean_raw, *mean_bias, *meas;             // raw means [n][z_dim], the mean layer's bias [z_dim], measurements [n][din - k z_dim]
    float* hist; const int *lanes, *first;                // [n_lanes][k - 1][z_dim]; [n] each
    const float *obs_mean, *obs_inv_std; float clip;      // NULL: not normalised
    float *sstate, *older;                                // [n][din]; [n][(k - 1) z_dim] or NULL
    const int* table_rows; long long n_table_rows; float *tab_states, *tab_raw_states;
    int n, z_dim, k, din, n_lanes, advance;
};

constexpr int ROLL_STACK_THREADS = 128, ROLL_STACK_REGS = 8;     // 128 x 8 = 1024 columns: MI_ROLLOUT_MAX_STACK latents of 64 and nothing else, or fewer and measurements

__global__ __launch_bounds__(ROLL_STACK_THREADS) void rollout_stack_kernel(const RollStackParams p) {
    const long long e = blockIdx.x;
    if (e >= p.n) return;                                 // (block-uniform)
    const int Z = p.z_dim, KZ = p.k * p.z_dim, HZ = KZ - Z, n_meas = p.din - KZ;
    const float* z = p.mean_raw + e * Z;
    const long long ms = e * n_meas - KZ;                 // measurement j - KZ of environment e is p.meas[ms + j]
    const int lane = p.lanes[e];
    const bool in_hist = lane >= 0 && lane < p.n_lanes;
    const bool first = !in_hist || p.first[e] != 0;
    float* h = p.hist + (in_hist ? (long long)lane * HZ : 0);
    float *tab = nullptr, *tab_raw = nullptr;
    if (p.table_rows) {
        const long long r = p.table_rows[e];
        if (r >= 0 && r < p.n_table_rows) {
            tab = p.tab_states + r * p.din;
            if (p.obs_mean) tab_raw = p.tab_raw_states + r * p.din;
        }
    }
    float* dst = p.sstate + e * p.din;
    float* old = p.older ? p.older + e * HZ : nullptr;
    float s[ROLL_STACK_REGS];
#pragma unroll
    for (int i = 0; i < ROLL_STACK_REGS; ++i) {
        const int j = threadIdx.x + i * ROLL_STACK_THREADS;
        s[i] = 0.f;
        if (j >= p.din) continue;
        if (j < KZ) {
            const int c = j < Z ? j : j % Z;
            if (j < Z || first) s[i] = z[c] + p.mean_bias[c];
            else s[i] = h[j - Z];
        } else {
            s[i] = p.meas[ms + j];
        }
        const float v = p.obs_mean ? obs_normalize(s[i], p.obs_mean[j], p.obs_inv_std[j], p.clip) : s[i];
        dst[j] = v;
        if (tab) tab[j] = v;
        if (tab_raw) tab_raw[j] = s[i];
        if (old && j >= Z && j < KZ) old[j - Z] = s[i];
    }
    __syncthreads();
    if (!p.advance || !in_hist) return;
#pragma unroll
    for (int i = 0; i < ROLL_STACK_REGS; ++i) {
        const int j = threadIdx.x + i * ROLL_STACK_THREADS;
        if (j < HZ) h[j] = s[i];
    }
}

}  // namespace mi

using namespace mi;

static int fill_conv1(RollConv1Params& c, const unsigned char* frame, const float* w, const float* bias, float* out, int IH, int IW, int Cs, int KH, int KW, int N, const MiZeroList* zero) {
    const int OH = (IH - KH) / 2 + 1, OW = (IW - KW) / 2 + 1;
    c = RollConv1Params{};
    c.frame = frame; c.w = w; c.bias = bias; c.out = out; c.IH = IH; c.IW = IW; c.Cs = Cs; c.OW = OW; c.M = OH * OW; c.N = N; c.KW = KW; c.K = KH * KW * Cs;
    if (zero) c.z = *zero;
    if (N > 32 || c.K > 48) return mi_fail(MI_ERR_SHAPE, "rollout conv1: at most 32 output channels and 48 patch values");
    return MI_OK;
}

int mi_rollout_conv1(hipStream_t st, const unsigned char* frame, const float* w, const float* bias, float* out, int IH, int IW, int Cs, int KH, int KW, int N, const MiZeroList* zero) {
    RollConv1Params c;
    int rc = fill_conv1(c, frame, w, bias, out, IH, IW, Cs, KH, KW, N, zero);
    if (rc != MI_OK) return rc;
    if (KW * Cs == 12) hipLaunchKernelGGL(rollout_conv1_kernel<12>, dim3((c.M + 127) / 128), dim3(256), 0, st, c);
    else hipLaunchKernelGGL(rollout_conv1_kernel<0>, dim3((c.M + 127) / 128), dim3(256), 0, st, c);
    return mi_check_launch("rollout_conv1_kernel");
}

static int log2_exact(int v) { int s = 0; while ((1 << s) < v) ++s; return (1 << s) == v ? s : -1; }

static int fill_conv(RollConvParams& p, dim3& g, const float* x, const float* x_bias, int IH, int IW, int C, const float* w, int ldw, int N, int KH, int KW, float* out_raw, int flat_k) {
    p = RollConvParams{};
    p.x = x; p.x_bias = x_bias; p.w = w; p.ldw = ldw; p.out = out_raw; p.IW = IW; p.C = C; p.N = N; p.KW = KW; p.flat = flat_k > 0 ? 1 : 0;
    p.relu = x_bias ? 1 : 0; p.c_shift = log2_exact(C);
    if (C % 4 != 0) return mi_fail(MI_ERR_SHAPE, "rollout conv: channels must be a multiple of 4");
    int ny;
    if (p.flat) {
        p.M = 1; p.OW = 1; p.K = flat_k; ny = 1;
        if (p.c_shift < 0 && C < flat_k) return mi_fail(MI_ERR_SHAPE, "rollout conv: a flattened input needs a power-of-two channel count");
    } else { const int OH = (IH - KH) / 2 + 1; p.OW = (IW - KW) / 2 + 1; p.M = OH * p.OW; p.K = KH * KW * C; ny = (p.M + 31) / 32; }
    p.vec = 1;
    if (p.flat && (flat_k & 3)) return mi_fail(MI_ERR_SHAPE, "rollout conv: the flattened input must be a multiple of 4 long");
    const long long xb = (p.flat ? (long long)flat_k : (long long)IH * IW * C) * 4, wb = (long long)p.K * ldw * 4, ob = (long long)p.M * N * 4;
    if (xb >= 0x40000000ll || wb >= 0x40000000ll || ob >= 0x40000000ll) return mi_fail(MI_ERR_SHAPE, "rollout conv: operand beyond 1 GiB");
    p.x_bytes = (unsigned)xb; p.xb_bytes = x_bias ? (unsigned)C * 4u : 0u; p.tail_bytes = 0; p.w_bytes = (unsigned)wb; p.out_bytes = (unsigned)ob;
    g = dim3((N + 31) / 32, ny, (p.K + 255) / 256);
    return MI_OK;
}

int mi_rollout_conv(hipStream_t st, const float* x, const float* x_bias, int IH, int IW, int C, const float* w, int ldw, int N, int KH, int KW, float* out_raw, int flat_k) {
    RollConvParams p; dim3 g;
    int rc = fill_conv(p, g, x, x_bias, IH, IW, C, w, ldw, N, KH, KW, out_raw, flat_k);
    if (rc != MI_OK) return rc;
    launch_conv(st, g, p);
    return mi_check_launch("rollout_conv_kernel");
}

// the two trunk layers as split-K stages: state = [mean_raw + mean_bias | measurements] -> layer 1 -> layer 2, raw sums into the zeroed q.h1 / q.h2
static void fill_trunks(RollConvParams& l1, dim3& g1, RollConvParams& l2, dim3& g2, const PpoFusedParams& q, const float* mean_raw, const float* mean_bias, int z_dim, const float* measurements) {
    RollConvParams p = {};
    p.flat = 1; p.M = 1; p.OW = 1; p.KW = 1; p.c_shift = -1;
    p.x = mean_raw; p.x_bias = mean_bias; p.x_tail = measurements; p.split = z_dim; p.relu = 0; p.C = q.din; p.K = q.din;
    p.w = q.theta + q.off[0]; p.ldw = q.H1; p.N = q.H1; p.out = q.h1;
    p.x_net = 0; p.xb_net = 0; p.w_net = q.off[7] - q.off[0]; p.out_net = q.H1;
    p.vec = 0; p.x_bytes = (unsigned)z_dim * 4u; p.xb_bytes = (unsigned)z_dim * 4u; p.tail_bytes = (unsigned)(q.din - z_dim) * 4u;
    p.w_bytes = (unsigned)q.din * (unsigned)q.H1 * 4u; p.out_bytes = (unsigned)q.H1 * 4u;
    l1 = p; g1 = dim3((q.H1 + 31) / 32, 2, (p.K + 255) / 256);
    p.x = q.h1; p.x_bias = q.theta + q.off[1]; p.x_tail = nullptr; p.split = 0; p.relu = 1; p.C = q.H1; p.K = q.H1;
    p.w = q.theta + q.off[2]; p.ldw = q.H2; p.N = q.H2; p.out = q.h2;
    p.x_net = q.H1; p.xb_net = q.off[8] - q.off[1]; p.w_net = q.off[9] - q.off[2]; p.out_net = q.H2;
    p.vec = 1; p.x_bytes = (unsigned)q.H1 * 4u; p.xb_bytes = (unsigned)q.H1 * 4u; p.tail_bytes = 0;
    p.w_bytes = (unsigned)q.H1 * (unsigned)q.H2 * 4u; p.out_bytes = (unsigned)q.H2 * 4u;
    l2 = p; g2 = dim3((q.H2 + 31) / 32, 2, (p.K + 255) / 256);
}

static void fill_head(RollHeadParams& h, const PpoFusedParams& q, const float* mean_raw, const float* mean_bias, int z_dim, const float* noise, int greedy, float* out) {
    h = RollHeadParams{};
    h.Wm = q.theta + q.off[4]; h.bm = q.theta + q.off[5]; h.logstd = q.theta + q.off[6]; h.b2p = q.theta + q.off[3]; h.b2v = q.theta + q.off[10];
    h.Wv = q.theta + q.off[11]; h.bv = q.theta + q.off[12]; h.low = q.low; h.high = q.high;
    h.h2raw = q.h2; h.mean_raw = mean_raw; h.mean_bias = mean_bias; h.noise = noise; h.mean_out = q.mean_out; h.out = out;
    h.A = q.A; h.H2 = q.H2; h.z_dim = z_dim; h.greedy = greedy;
}

int mi_rollout_policy(hipStream_t st, const PpoFusedParams& q, const float* mean_raw, const float* mean_bias, int z_dim, const float* measurements,
                      const float* noise, int greedy, float* out) {
    if (q.A < 1 || q.A > 8) return mi_fail(MI_ERR_ARG, "rollout step: 1 <= num_actions <= 8");
    if (q.H1 % 4 != 0) return mi_fail(MI_ERR_SHAPE, "rollout step: hidden sizes must be multiples of 4");
    RollConvParams l1, l2; dim3 g1, g2; RollHeadParams h;
    fill_trunks(l1, g1, l2, g2, q, mean_raw, mean_bias, z_dim, measurements);
    fill_head(h, q, mean_raw, mean_bias, z_dim, noise, greedy, out);
    launch_conv(st, g1, l1);
    launch_conv(st, g2, l2);
    if (q.A <= 2) hipLaunchKernelGGL(rollout_head_kernel<2>, dim3(1), dim3(256), 0, st, h);
    else hipLaunchKernelGGL(rollout_head_kernel<8>, dim3(1), dim3(256), 0, st, h);
    return mi_check_launch("rollout_policy");
}


// ---- the batched step: n environments per launch (mi_rollout_step_batch) ----

int mi_rollout_conv1_batch(hipStream_t st, const unsigned char* frames, const float* w, const float* bias, float* out, int IH, int IW, int Cs, int KH, int KW, int N, int n,
                           const MiZeroList* zero) {
    RollConv1BatchParams c;
    int rc = fill_conv1(c, frames, w, bias, out, IH, IW, Cs, KH, KW, N, zero);
    if (rc != MI_OK) return rc;
    c.OHW = c.M; c.frame_stride = (unsigned)(IH * IW * Cs);
    const long long fb = (long long)n * c.frame_stride, ob = (long long)n * c.OHW * N * 4;
    if (fb >= 0x40000000ll || ob >= 0x40000000ll) return mi_fail(MI_ERR_SHAPE, "rollout conv1: operand beyond 1 GiB");
    c.M = n * c.OHW;
    const dim3 g((c.M + 127) / 128);
    // the two-byte loads of the 12-byte patch row need every frame to start on an even byte
    if (KW * Cs == 12 && (c.frame_stride & 1u) == 0 && (((uintptr_t)frames) & 1) == 0) hipLaunchKernelGGL(rollout_conv1_batch_kernel<12>, g, dim3(256), 0, st, c);
    else hipLaunchKernelGGL(rollout_conv1_batch_kernel<0>, g, dim3(256), 0, st, c);
    return mi_check_launch("rollout_conv1_batch_kernel");
}

// conv (flat_k = 0): x [n][IH,IW,C] -> raw sums [n OH OW][N].  flat (flat_k > 0): x [n][flat_k] -> raw sums [n][N]
int mi_rollout_conv_batch(hipStream_t st, const float* x, const float* x_bias, int IH, int IW, int C, const float* w, int ldw, int N, int KH, int KW, float* out_raw, int flat_k, int n) {
    RollConvBatchParams p; dim3 g;
    int rc = fill_conv(p, g, x, x_bias, IH, IW, C, w, ldw, N, KH, KW, out_raw, flat_k);
    if (rc != MI_OK) return rc;
    p.OHW = p.M; p.img_stride = (unsigned)(IH * IW * C); p.row_tiles = (n + 31) / 32; p.x_row = (unsigned)flat_k; p.t_row = 0;
    const long long xb = (long long)n * p.x_bytes, ob = (long long)n * p.out_bytes;
    if (xb >= 0x40000000ll || ob >= 0x40000000ll) return mi_fail(MI_ERR_SHAPE, "rollout conv: operand beyond 1 GiB");
    p.x_bytes = (unsigned)xb; p.out_bytes = (unsigned)ob; p.M = n * p.OHW;
    g.y = p.flat ? p.row_tiles : (p.M + 31) / 32;
    if (g.y > 65535u) return mi_fail(MI_ERR_SHAPE, "rollout conv: too many row tiles");
    launch_conv_batch(st, g, p);
    return mi_check_launch("rollout_conv_batch_kernel");
}

// the two trunk layers of n environments as batched split-K stages: rows run over the environments, raw sums in q.h1 / q.h2 as [net][n][H]; grid.y = 2 nets x row tiles
static int fill_trunks_batch(RollConvBatchParams& l1, dim3& g1, RollConvBatchParams& l2, dim3& g2, const PpoFusedParams& q, const float* mean_raw, const float* mean_bias, int z_dim,
                             const float* measurements, int n) {
    if (q.A < 1 || q.A > 8) return mi_fail(MI_ERR_ARG, "rollout step: 1 <= num_actions <= 8");
    if (q.H1 % 4 != 0) return mi_fail(MI_ERR_SHAPE, "rollout step: hidden sizes must be multiples of 4");
    if ((long long)n * (q.H1 > q.H2 ? q.H1 : q.H2) * 4 >= 0x40000000ll || (long long)n * q.din * 4 >= 0x40000000ll) return mi_fail(MI_ERR_SHAPE, "rollout step: operand beyond 1 GiB");
    RollConvParams b1, b2;
    fill_trunks(b1, g1, b2, g2, q, mean_raw, mean_bias, z_dim, measurements);
    const unsigned un = (unsigned)n;
    static_cast<RollConvParams&>(l1) = b1; static_cast<RollConvParams&>(l2) = b2;
    l1.OHW = l2.OHW = 1; l1.img_stride = l2.img_stride = 0; l1.row_tiles = l2.row_tiles = (n + 31) / 32;
    l1.M = l2.M = n;
    l1.x_row = (unsigned)z_dim; l1.t_row = (unsigned)(q.din - z_dim); l1.x_bytes *= un; l1.tail_bytes *= un; l1.out_bytes *= un; l1.out_net = (long long)n * q.H1;
    l2.x_row = (unsigned)q.H1; l2.t_row = 0; l2.x_bytes *= un; l2.out_bytes *= un; l2.x_net = (long long)n * q.H1; l2.out_net = (long long)n * q.H2;
    g1.y = g2.y = 2 * l1.row_tiles;
    return MI_OK;
}

// trunk layer 1 re-aimed at finished state rows [n][din]: the same rollout_conv_batch_kernel<3> with x = rows, split = K = din, no bias and no tail (both
// descriptors empty: every load of them returns 0.0)
static void layer1_reads_rows(RollConvBatchParams& l1, const float* rows, int din, int n) {
    l1.x = rows; l1.x_bias = nullptr; l1.x_tail = nullptr; l1.split = din;
    l1.x_row = (unsigned)din; l1.t_row = 0;
    l1.x_bytes = (unsigned)n * (unsigned)din * 4u; l1.xb_bytes = 0; l1.tail_bytes = 0;
}

int mi_rollout_fail(int code, const char* who, const char* text) {
    char msg[192];
    snprintf(msg, sizeof(msg), "%s: %s", who, text);
    return mi_fail(code, msg);
}

int mi_rollout_call_check(const MiRolloutCall& c, const void* frames, const void* scratch) {
    const auto fail = [&c](const char* text) { return mi_rollout_fail(MI_ERR_ARG, c.who, text); };
    const bool norm = c.must_normalise || c.obs_mean;
    if (!frames || !c.out || !scratch || (c.n_meas > 0 && !c.measurements) || (!c.greedy && !c.noise)) return fail("missing buffers");
    if ((c.must_record || c.table_rows) &&
        (!c.table_rows || c.n_table_rows < 1 || (c.value_only ? !c.tab_final_values : (!c.tab_states || !c.tab_actions || !c.tab_values || (norm && !c.tab_raw_states)))))
        return mi_rollout_fail(MI_ERR_ARG, c.who_rec, "missing tables");
    if (c.stacked) {
        if (c.latent_stack < 2 || c.latent_stack > MI_ROLLOUT_MAX_STACK) return fail("2 <= latent_stack <= MI_ROLLOUT_MAX_STACK");
        if (!c.hist || !c.lanes || !c.first || !c.sstate || c.n_lanes < 1) return fail("missing hist / lanes / first / sstate");
        if (((uintptr_t)c.sstate) & 15) return fail("sstate must be 16-byte aligned");
        if (c.obs_mean && (!c.obs_inv_std || !(c.obs_clip > 0.f))) return fail("obs_inv_std is missing or obs_clip is not a positive value (+inf: never clamp)");
        if (!c.obs_mean && (c.obs_inv_std || c.tab_raw_states)) return fail("obs_inv_std and tab_raw_states are NULL where obs_mean is");
    } else if (norm) {
        if (!c.obs_mean || !c.obs_inv_std || !c.nstate) return fail("missing obs_mean / obs_inv_std / nstate");
        if (((uintptr_t)c.nstate) & 15) return fail("nstate must be 16-byte aligned");
        if (!(c.obs_clip > 0.f)) return fail("obs_clip is a positive value (+inf: never clamp)");
    } else if (c.obs_inv_std || c.nstate || c.tab_raw_states) {
        return fail("obs_inv_std, nstate and tab_raw_states are NULL where obs_mean is");
    }
    if (c.n < 1 || c.n > MI_ROLLOUT_MAX_ENVS) return fail("1 <= n <= MI_ROLLOUT_MAX_ENVS");
    return MI_OK;
}

int mi_rollout_call_prepare(const MiRolloutCall& c, void* ppo_h, const float* mean_raw, int z_dim, PpoFusedParams* q, MiZeroList* zero) {
    const int rc = mi_ppo_internal_fill(ppo_h, q, mean_raw, 1);
    if (rc != MI_OK) return rc;
    if (c.stacked) {
        if ((long long)c.latent_stack * z_dim + c.n_meas != q->din) return mi_rollout_fail(MI_ERR_SHAPE, c.who, "latent_stack x z_dim + measurements must equal the policy's input size");
        if (q->din > ROLL_STACK_THREADS * ROLL_STACK_REGS) return mi_rollout_fail(MI_ERR_SHAPE, c.who, "at most 1024 inputs");
    } else if (q->din != z_dim + c.n_meas) {
        return mi_rollout_fail(MI_ERR_SHAPE, c.who, "z_dim + measurements must equal the policy's input size");
    }
    if (q->A > 8) return mi_rollout_fail(MI_ERR_ARG, c.who, "at most 8 actions");
    if (mi_ppo_internal_fill(ppo_h, q, mean_raw, c.n) != MI_OK) return mi_rollout_fail(MI_ERR_ARG, c.who, "n exceeds the PPO engine's max_batch");
    const long long nets = c.value_only ? 1 : 2, skip = 2 - nets;          // [net][n][H]: both nets, or net 1 (the value net's half) alone
    zero->p[1] = q->h1 + skip * c.n * q->H1; zero->n[1] = nets * c.n * q->H1;
    zero->p[2] = q->h2 + skip * c.n * q->H2; zero->n[2] = nets * c.n * q->H2;
    return MI_OK;
}

// trunks and heads of n environments: mean_raw [n][z_dim], measurements [n][din - z_dim], noise [n][A]; raw sums in q.h1 / q.h2 as [net][n][H]
int mi_rollout_call_finish(hipStream_t st, const MiRolloutCall& c, const PpoFusedParams& q, const float* mean_raw, const float* mean_bias, int z_dim) {
    RollConvBatchParams l1, l2; dim3 g1, g2;
    const int n = c.n, rc = fill_trunks_batch(l1, g1, l2, g2, q, mean_raw, mean_bias, z_dim, c.measurements, n);
    if (rc != MI_OK) return rc;
    const int* state_rows = c.value_only ? nullptr : c.table_rows;       // the value-only call records no state: the final observation of a truncated episode is no step
    if (c.stacked) {                                     // the stack launch (it normalises as well), and trunk layer 1 re-aimed at the rows it wrote
        const RollStackParams p = {mean_raw, mean_bias, c.measurements, c.hist, c.lanes, c.first, c.obs_mean, c.obs_inv_std, c.obs_clip, c.sstate, c.older,
                                   state_rows, c.n_table_rows, c.tab_states, c.tab_raw_states, n, z_dim, c.latent_stack, q.din, c.n_lanes, c.advance};
        hipLaunchKernelGGL(rollout_stack_kernel, dim3(n), dim3(ROLL_STACK_THREADS), 0, st, p);
        layer1_reads_rows(l1, c.sstate, q.din, n);
    } else if (c.obs_mean) {                             // the normalise launch, likewise
        const RollObsNormParams p = {mean_raw, mean_bias, c.measurements, c.obs_mean, c.obs_inv_std, c.obs_clip, c.nstate, state_rows, c.n_table_rows, c.tab_states, n, z_dim, q.din};
        hipLaunchKernelGGL(rollout_obs_norm_kernel, dim3(n), dim3(128), 0, st, p);
        layer1_reads_rows(l1, c.nstate, q.din, n);
    }
    if (c.value_only) {                                  // the VALUE trunk alone: the operands moved to net 1 and half the grid (the policy net's half of q.h1 / q.h2 is neither cleared, written nor read)
        l1.w += l1.w_net; l1.out += l1.out_net;                                                // (layer 1's x / bias strides are 0: both nets read the one state)
        l2.x += l2.x_net; l2.x_bias += l2.xb_net; l2.w += l2.w_net; l2.out += l2.out_net;
        g1.y = l1.row_tiles; g2.y = l2.row_tiles;                                              // blockIdx.y / row_tiles = 0: the kernels' "net 0" is the value net
    }
    launch_conv_batch(st, g1, l1);
    launch_conv_batch(st, g2, l2);
    if (c.value_only) {
        // table_rows NULL (the MLP entries): the value heads read one int per environment whatever the tables are; with n_table_rows = 0 no row lies inside the table and
        // nothing is stored, so the list may be any n readable ints: the raw means
        const RollValueParams v = {l2.out, q.theta + q.off[10], q.theta + q.off[11], q.theta + q.off[12], q.H2, c.table_rows ? c.table_rows : (const int*)mean_raw,
                                   c.table_rows ? c.n_table_rows : 0, c.out, c.tab_final_values};
        hipLaunchKernelGGL(rollout_value_rec_kernel, dim3(n), dim3(256), 0, st, v);
        return mi_check_launch("rollout_value_batch");
    }
    RollHeadParams h;
    fill_head(h, q, mean_raw, mean_bias, z_dim, c.noise, c.greedy, c.out);
    if (c.table_rows) {                                  // the recording heads store action, value and the raw state (stacked: the stack kernel has written the rows already)
        const RollRecParams t = {c.table_rows, c.n_table_rows, c.measurements, q.din - z_dim, q.din, c.stacked ? nullptr : (c.obs_mean ? c.tab_raw_states : c.tab_states),
                                 c.tab_actions, c.tab_values};
        if (q.A <= 2) hipLaunchKernelGGL(rollout_head_rec_kernel<2>, dim3(n), dim3(256), 0, st, h, n, t);
        else hipLaunchKernelGGL(rollout_head_rec_kernel<8>, dim3(n), dim3(256), 0, st, h, n, t);
        return mi_check_launch("rollout_policy_batch_rec");
    }
    if (q.A <= 2) hipLaunchKernelGGL(rollout_head_batch_kernel<2>, dim3(n), dim3(256), 0, st, h, n);
    else hipLaunchKernelGGL(rollout_head_batch_kernel<8>, dim3(n), dim3(256), 0, st, h, n);
    return mi_check_launch("rollout_policy_batch");
}
