// mi_internal.hpp — error plumbing shared by the launchers (not part of the public C ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include "tuning.hpp"                              // mi::knob(K_...): every launcher reads its knobs from the one table

enum { MI_F32 = 0, MI_BF16 = 1, MI_BF16X3 = 2 };   // MI_BF16X3: split storage (hi | lo bf16 halves per 4-byte element), common.hpp
enum { MI_OK = 0, MI_ERR_ARG = -1, MI_ERR_SHAPE = -2, MI_ERR_LAUNCH = -3, MI_ERR_STATE = -4 };

// A kernel launch that carries the caller's completion event ON ITS OWN DISPATCH PACKET (hipExtLaunchKernelGGL's stop event) instead of a separate
// hipEventRecord marker behind it: the VAE engine's backward pass hands every gradient tensor from the caller's stream to the filter-gradient stream, and each
// marker packet cost the producing queue ~6-8 us of bubble (profiles/r03_d, dispatch timeline; round 4).  The engine sets mi_tl_stop_event right before the
// layer call whose (single) kernel produces the tensor; the first MI_LAUNCH of that call consumes it.  Unset (the default): a plain launch.
extern thread_local hipEvent_t mi_tl_stop_event;
#define MI_LAUNCH(kernel, grid, block, shmem, stream, ...) do { \
        if (mi_tl_stop_event) { const hipEvent_t ev__ = mi_tl_stop_event; mi_tl_stop_event = nullptr; \
            hipExtLaunchKernelGGL(kernel, grid, block, shmem, stream, nullptr, ev__, 0, __VA_ARGS__); } \
        else hipLaunchKernelGGL(kernel, grid, block, shmem, stream, __VA_ARGS__); } while (0)

const void* mi_rwconv_take_wfrag();             // rwconv.hip: returns and clears this thread's mi_rwconv_next_weights_fragment_ordered announcement (called first thing by the entries it applies to)
bool mi_enc12_eligible(int dtype, int B, int FH, int FW);   // enc12.hip: mi_conv2d_enc12_fwd takes calls of this storage type / batch / frame size (before its alignment checks)
int mi_fail(int code, const char* msg);          // records msg (thread-local) and returns code
int mi_check_launch(const char* what);           // hipGetLastError() -> MI_OK / MI_ERR_LAUNCH

// ---- Slab sums that a backward pass issues LATER than the kernel that wrote the slabs (conv_ops.hip).  The pass owns the two lists below for its own length (on its
// stack) and hands them down the filter-gradient calls in a MiWgradCtx; nothing of this is per-thread or per-process state.  Each list is created with the ONE stream it
// will be flushed on; a list that goes out of scope with jobs in it launches nothing.
//
// The small ordered slab sums (reduce_small_fused_kernel): out[0 .. n) += (overwrite: =) sum_k slabs[k * stride + i] in a fixed order.
//   * add (mi_reduce_slabs with the list): a job of the list's stream is recorded -- its slabs must stay untouched until the flush; a job of ANY OTHER stream is launched
//     at once on its own stream (one launch of the same kernel), never flushed later on a stream that did not wait for its slabs.
//   * a full list (MI_SMALL_SUMS_MAX jobs) is issued as it is and recording goes on.
//   * mi_small_sums_flush: ONE launch on the list's stream; the list is empty afterwards and may go on recording.
struct MiSlabSum { const float* slabs; float* out; long long stride, n; int nslab, overwrite; };
constexpr int MI_SMALL_SUMS_MAX = 12;            // the jobs of one launch (= SR_MAX of tapwgrad_tile.hpp)
struct MiSmallSums {
    hipStream_t stream; int njobs; MiSlabSum job[MI_SMALL_SUMS_MAX];
    explicit MiSmallSums(void* st) : stream((hipStream_t)st), njobs(0) {}
};
int mi_small_sums_flush(MiSmallSums* l);
// The tiled reduces of the raw-staged filter-gradient kernel (try_tapwgrad) and the folds of its split-storage form (try_tapwgrad_split).
//   * a reduce (a fold) of a call on the list's stream is recorded, up to 16 of each -- every layer then needs its OWN scratch region until the flush; past 16, or from
//     any other stream, it is launched right behind its kernel.
//   * mi_tiled_reduces_flush: the recorded reduces (one launch each for 1 or more than TW_MAX_FUSED of them, else one reduce_fused_kernel), then -- only where folds are
//     recorded -- the jobs of `small` if that list is on the same stream (the folds read its sums), then the folds.  Recording may go on afterwards.
struct MiTiledReduces {
    hipStream_t stream; int nreduce, nfold;
    alignas(16) unsigned char store[11 << 10];   // 16 reduces, 16 folds, the fused launch's argument block: types of the kernel headers, which this header does not pull in (conv_ops.hip)
    explicit MiTiledReduces(void* st) : stream((hipStream_t)st), nreduce(0), nfold(0) {}
};
int mi_tiled_reduces_flush(MiTiledReduces* l, MiSmallSums* small);
// What a filter-gradient call takes from the pass that issues it.  NULL, or NULL lists: what a layer-op call from outside gets -- every reduce right behind its kernel.
// (mi_tl_stop_event above and mi_rwconv_next_weights_fragment_ordered are hidden arguments of the same kind; they reach every launcher and were left as they are on purpose.)
struct MiWgradCtx {
    MiTiledReduces* tiled;                       // or NULL
    MiSmallSums* small;                          // or NULL.  The encoder-head and decoder-tail sums take reduce_small_fused_kernel whenever a list is given, also one of another stream
    int slab_bf16;                               // != 0: the raw-staged kernels round their partial-sum slabs to bf16 (the engine's bf16 backward); 0: K_SLAB_BF16_DEFAULT
    int bias_rows;                               // != 0: a raw-staged filter gradient with ONE position split sums its bias partial rows through the scratch in a fixed order
};                                               //       instead of atomics.  A NULL context follows mi_tapwgrad_bias_rows, this thread's public switch (mi355_carla.h)
// the entries of mi355_carla.h that issue slab sums, with the context (the public ones pass NULL; C linkage as theirs, defined next to them)
extern "C" {
int mi_conv2d_nhwc_wgrad_ctx(void* stream, int dtype, const void* x, const int* frame_idx, int x_is_f32, int B, int IH, int IW, int Cin, const void* dy, int KH, int KW, int Cout,
                             float* dw, void* scratch, long long scratch_bytes, float* dbias, const MiWgradCtx* ctx);
int mi_deconv2d_nhwc_wgrad_ctx(void* stream, int dtype, const void* dy, int B, int OH, int OW, int Cout, const void* x, int KH, int KW, int Cin,
                               float* dw, void* scratch, long long scratch_bytes, float* dbias, const MiWgradCtx* ctx);
int mi_gemm_wgrad_bias_ctx(void* stream, int dtype, const void* a, const void* dy, int M, int K, int N, float* dw, float* dbias, void* scratch, long long scratch_bytes, int overwrite, const MiWgradCtx* ctx);      // mi_gemm_wgrad_bias_set (and through it _ws, _bias_ws)
int mi_gemm_wgrad_bias_pair_ctx(void* stream, int dtype, const void* a0, const void* dy0, int M0, int K0, int N0, float* dw0, float* db0, void* scratch0, long long scratch_bytes0,
                                const void* a1, const void* dy1, int M1, int K1, int N1, float* dw1, float* db1, void* scratch1, long long scratch_bytes1, const MiWgradCtx* ctx);
int mi_colsum_ctx(void* stream, int dtype, const void* x, long long M, int N, float* out, void* scratch, long long scratch_bytes, const MiWgradCtx* ctx);      // elementwise.hip
int mi_deconv2d_tail_reduce_ctx(void* stream, const void* scratch, int n_partial, float* dw, const MiWgradCtx* ctx);
int mi_conv2d_head_bwd_fused_ctx(void* stream, int dtype, const void* frames, int frames_fmt, const int* frame_idx, int B, int FH, int FW, const void* dy2, const void* w2,
                                 const void* bits_act1, float* dw1, float* db1, void* scratch, long long scratch_bytes, int* n_blocks, const MiWgradCtx* ctx);      // enchead.hip
}

// register-weight kernel of the thin gather-form layers (rwconv.hip): 1 launched, 0 not eligible, < 0 error
// wfrag: the layer's weights in fragment order (mi_rwconv_take_wfrag), or NULL
int mi_try_rwconv_gather(hipStream_t st, int dtype, const void* a, const void* w, int B, int IH, int IW, int C, int OH, int OW, int N,
                         int KH, int KW, void* out, const float* bias, const void* mask, int relu, const void* mask_bits, void* bits_out, const void* wfrag);
int mi_try_rwconv_conv(hipStream_t st, int dtype, const void* a, const void* w, int B, int IH, int IW, int C, int OH, int OW, int N,
                       int KH, int KW, int ldb, void* out, const float* bias, const void* mask, int relu, const void* wfrag);   // rwconv.hip, conv form (32 -> 64 channels)
void mi_get_trace(long long** buf, int* cap);     // the debug stamp buffer of mi_debug_set_trace

// out[0 .. n) += sum over nslab slabs of slabs[k * stride + i] (reduce_small_fused_kernel, tapwgrad_tile.hpp; fixed summation order, no atomics) -- conv_ops.hip
// overwrite: out = sum.  list: NULL = one launch right here; else MiSmallSums' add rule above
int mi_reduce_slabs(hipStream_t st, const float* slabs, long long stride, int nslab, long long n, float* out, int overwrite = 0, MiSmallSums* list = nullptr);

// global-norm gradient clipping in front of TF ApplyAdam (elementwise.hip; the PPO engine).  mi_grad_sumsq: sum of (double)g * (double)g over `count` tensors of a
// flat fp32 buffer (offsets in floats, multiples of 4; what lies between the tensors is not read) as MI_GRAD_NORM_BLOCKS ordered block partials.  mi_grad_norm_finish:
// partials -> clip_out {norm, scale, max_norm, 0} (16-byte aligned), scale = (float)(max_norm / norm) where the norm is finite and above max_norm, else 1.
// mi_adam_tf_flat_clipped: mi_adam_tf_flat on __fmul_rn(g, scale), scale formed from the partials by every block; block 0 also stores clip_out.  No atomics.
#define MI_GRAD_NORM_BLOCKS 64
#define MI_GRAD_NORM_MAX_TENSORS 16
int mi_grad_sumsq(hipStream_t st, const float* grad, const long long* off, const long long* size, int count, double* partial);
int mi_grad_norm_finish(hipStream_t st, const double* partial, float max_norm, float* clip_out);
int mi_adam_tf_flat_clipped(hipStream_t st, float* param, float* m, float* v, float* grad, long long n, float alpha, float beta1, float beta2, float epsilon,
                            const double* partial, float max_norm, float* clip_out, int clear_grad);
