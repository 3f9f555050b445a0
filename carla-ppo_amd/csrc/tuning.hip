// tuning.hip — THE table of tuning knobs (tuning.hpp): one row per knob, the only getenv of the library, and mi_set_tuning as a lookup of the key's row.
// DESIGN.md section 7 lists the same rows for readers; a knob is added here, there, and nowhere else.
#include <limits.h>
#include <stdlib.h>
#include "mi_internal.hpp"
#include "mi355_carla.h"

namespace mi {
namespace {

enum Parse : char {       // the environment string e of a row (unset: the default)
    P_NONE,               // no environment name
    P_ON,                 // on unless e[0] == '0'
    P_OFF,                // off unless e[0] == '1'
    P_OFF_PER_CALL,       // as P_OFF, but parsed by every read (knob_env_now): tools set and delete it between calls in one process
    P_INT,                // atoi(e), taken raw
    P_RANGE,              // atoi(e); outside lo .. hi: the default
    P_DWG_NST             // 4 for exactly 4, else 3
};
enum Set : char {         // what mi_set_tuning(key, v) stores
    S_NONE,               // no key
    S_RAW,                // v
    S_BOOL,               // v != 0
    S_CLAMP,              // v clamped to lo .. hi (NOT the environment's rule: MI355_RWCONV=7 gives the default 1, mi_set_tuning(13, 7) gives 2)
    S_DEF_OUTSIDE,        // v; outside lo .. hi: the default
    S_IGNORED             // nothing: the key of a removed knob, kept so that old callers do not fail
};
struct Row { Knob id; const char* env; int key, def; Parse parse; Set set; int lo, hi; };
constexpr int NOKEY = -1, MAXI = INT_MAX;

constexpr Row rows[K_COUNT] = {
    // ---- keyed knobs (the enumerator is the key) ----
    {K_GEMM2, "MI355_GEMM2", 0, 1, P_ON, S_BOOL},                                  // gemm2 (LDS-DMA tiles) for the wide layers; 0: the first-generation register-staged kernel (A/B, bisecting)
    {K_TAPCONV_MINBLOCKS, "MI355_TAPCONV_MINBLOCKS", 1, 300, P_INT, S_CLAMP, -1, MAXI},   // tapconv: least number of blocks (occupancy threshold) a layer needs to take it; -1: tapconv off (what MI355_TAPCONV=0 stores here)
    {K_WGRAD_DBG, nullptr, 2, 0, P_NONE, S_RAW},                                   // TIMING mask of the filter-gradient / tapconv kernels (wrong results, honest durations; tools/wgrad_ablate.py): 1 skip the output, 2-5 cheap DMA addresses
    {K_TAPWGRAD, "MI355_TAPWGRAD", 3, 1, P_ON, S_BOOL},                            // tapwgrad: bf16 filter gradients of the wide stride-2 layers on raw-staged slot tiles
    {K_NARROW, "MI355_NARROW", 4, 1, P_ON, S_BOOL},                                // the narrow-layer kernels (narrow_tile.hpp); off also switches the fused encoder head off
    {K_TAP_VARIANT, nullptr, 5, 0, P_NONE, S_RAW},                                 // tapconv tile: 0 auto, 1 big (256 x 96), 2 small (128 x 48)
    {K_TAP_DIRECT, nullptr, 6, 1, P_NONE, S_BOOL},                                 // tapconv epilogue: 1 registers -> 16-byte stores, 0 LDS-staged
    {K_TAPWGRAD_SPLIT, nullptr, 7, 1, P_NONE, S_BOOL},                             // 2 x 2-tap filter gradient with 8 pairs: a wave = (tap, position half), fewer LDS reads per MFMA; 0: the pair layout
    {K_KEY8_REMOVED, nullptr, 8, 0, P_NONE, S_IGNORED},                            // (was: persistent tapconv blocks, removed -- rwconv.hip is the persistent form that won); always 0
    {K_TAPWGRAD_BLOCKS, nullptr, 9, 256, P_NONE, S_CLAMP, 16, MAXI},               // tapwgrad: target number of blocks (position splits x block columns)
    {K_NW_BLOCK_WAVES, nullptr, 10, 12, P_NONE, S_RAW},                            // narrow_wgrad: waves per BLOCK (4 | 8 | 12) -- not MI355_NW_WAVES (K_NW_WAVES below), which sizes the grid
    {K_DENSE_WGRAD_BLOCKS, "MI355_DENSE_WGRAD_BLOCKS", 11, 256, P_INT, S_CLAMP, 1, MAXI},   // dense filter gradients: target block count (row splits)
    {K_TAP_MASK_PREFETCH, nullptr, 12, 1, P_NONE, S_BOOL},                         // tapconv: touch the ReluGrad-mask lines in the last main-loop step
    {K_RWCONV, "MI355_RWCONV", 13, 1, P_RANGE, S_CLAMP, 0, 2},                     // register-weight kernels (rwconv.hip): 0 off, 1 auto (where the grid fills the chip), 2 whenever the layer is eligible
    {K_TAPWGRAD_CW, nullptr, 14, 1, P_NONE, S_BOOL},                               // k = 5 filter gradient: class-wave layout (tapwgrad_cw_kernel); 0: the pair layout
    {K_RWCONV_CONV, "MI355_RWCONV_CONV", 15, 3, P_RANGE, S_CLAMP, 0, 3},           // conv form on the register-weight kernel: 0 off, 1 the k = 5 layer, 2 also 32 -> 64 channels k = 4, 3 also 64 -> 128 channels
    {K_RWCONV_BLOCKS, "MI355_RWCONV_BLOCKS", 16, 0, P_INT, S_CLAMP, 0, MAXI},      // register-weight kernels: persistent blocks per XCD, 0 = as many as stay resident (one, k = 4 gather: three, per CU)
    {K_GEMM2_TILE, "MI355_GEMM2_TILE", 17, 2, P_INT, S_RAW},                       // wide-output gemm2 layers: 0 auto (64 x 64 tiles on small grids), 1 always 64 x 64, 2 never, 3 always 128 x 128 (64 x 64 wave tiles: 1 KB of LDS reads per MFMA instead of 1.5)
    {K_SLAB_BF16_DEFAULT, nullptr, 18, 0, P_NONE, S_BOOL},                         // tapwgrad partial-sum slabs rounded to bf16 (half the slab traffic): the PROCESS DEFAULT of the layer-op entry points (off: exact fp32 partial sums),
                                                                                   // which a pass may override for its own calls (MiWgradCtx::slab_bf16) -- not MI355_SLAB_BF16 (K_SLAB_BF16 below), the engine's switch that sets that override
    {K_NW_DEPTH, "MI355_NW_DEPTH", 19, 3, P_INT, S_RAW},                           // narrow_wgrad (uint8 conv1 shape): steps in flight per wave (3 | 5 | 6)
    {K_GEMM2_STAGES, "MI355_GEMM2_STAGES", 20, 2, P_INT, S_RAW},                   // gemm2 128 x 64 tiles: LDS stages of the K pipeline (2 | 3 | 4)
    {K_X3_TAPWGRAD, "MI355_X3_TAPWGRAD", 21, 1, P_INT, S_RAW},                     // split-storage filter gradients on the doubled-channel bf16 kernel: 0 off, 1 conv2 / conv3 (default since round 5: 2.637 -> 2.595 ms per bf16x3 step, two interleaved pairs on one box;
        // round 4 measured no difference), 2 every eligible layer (2.870: the wide layers lose).  Measured per layer at batch 512 (us, doubled-channel bf16 kernel vs the first-generation split kernel):
        // conv2 125 / 164, conv3 122 / 136, deconv2 150 / 150, conv4 187 / 86, deconv1 227 / 91 -- the wide layers end up with 64 column blocks and four position splits
    {K_DWGS, "MI355_DWGS", 22, 1, P_ON, S_BOOL},                                   // LDS-free one-wave-per-tile dense filter gradient (dwgs_tile.hpp, round 5) for bf16 layers of up to 2048 tiles of 64 x 64
    {K_ENC12_DBG, nullptr, 23, 0, P_NONE, S_CLAMP, 0, MAXI},                       // TIMING mask of the fused encoder-head forward kernel (tools/enc12_ablate.py) -- results are wrong with any bit set; bit 4096: pick a product form by mask
    {K_TW_LDEC, "MI355_TW_LDEC", 24, 0, P_RANGE, S_DEF_OUTSIDE, 0, 3},             // raw-staged filter gradients: a step's DMA rows decoded once per wave, one row per lane (tapwgrad_tile.hpp, round 6).  bit 0: the 2 x 2-tap kernels, bit 1: the k = 5 class-wave kernel.
        // Default 0: once the product kernels lost their run-time debug branch the two forms are equal (0.7929 / 0.7932 / 0.7942 ms for 0 / 1 / 3)
    {K_DECTAIL_DBG, nullptr, 25, 0, P_NONE, S_RAW},                                // TIMING mask of the decoder tail's timing instantiation (wrong results)
    {K_DECTAIL_SPLIT5, "MI355_DECTAIL_SPLIT5", 26, 0, P_OFF, S_BOOL},              // decoder tail: the fifth slot group's loss shared by three waves (dectail_tile.hpp, round 6); measured neutral (74.4-77.4 vs 76.2-77.6 us alone, 0.8440 = 0.8440 ms per step): off
    // ---- environment only (A/B runs) ----
    {K_TAPCONV, "MI355_TAPCONV", NOKEY, 1, P_ON},                                  // 0: tapconv off -- stored as K_TAPCONV_MINBLOCKS = -1, and wins over MI355_TAPCONV_MINBLOCKS
    {K_GEMM2_SPLITK, "MI355_GEMM2_SPLITK", NOKEY, 1, P_ON},                        // split-K dense layers (raw fp32 slabs) on the LDS-DMA tiles instead of the first-generation kernel (round 4: the 38400-long reductions of the MlpVAE)
    {K_GEMM2_REMAP3, "MI355_GEMM2_REMAP3", NOKEY, 1, P_ON},                        // dense layers on gemm2: XCD-contiguous numbering of the whole grid; 0: x only, as for the convolutions
    {K_REDUCE_RY_CAP, "MI355_REDUCE_RY_CAP", NOKEY, 16, P_RANGE, S_NONE, 1, 64},   // tiled slab reduce: most slab chains per element -- fewer chains = longer contiguous pieces per slab and block, fewer blocks
                                                                                   // (16: 0.7900 / 0.7923 against 0.7929 / 0.7949 ms per step at 64, two interleaved A/B runs of four rounds)
    {K_NARROW_LEAN, "MI355_NARROW_LEAN", NOKEY, 1, P_ON},                          // 0: the first-generation narrow-layer kernels
    {K_NW_WAVES, "MI355_NW_WAVES", NOKEY, 12, P_INT},                              // narrow_wgrad: resident waves per CU the GRID is sized for (131 registers -> 3 per SIMD) -- not key 10 (waves per block)
    {K_TALLK, "MI355_TALLK", NOKEY, 1, P_ON},                                      // 0: the general split-K kernel for the latent-side layers
    {K_DECTAIL, "MI355_DECTAIL", NOKEY, 1, P_ON},                                  // fused decoder tail (dectail_tile.hpp): the engine plans by it, mi_deconv2d_tail_fused launches by it
    {K_DECTAIL_EDGE, "MI355_DECTAIL_EDGE", NOKEY, 1, P_ON},                        // decoder tail: tiles over the pixel grid, last slot row / column owned by the last tiles
    {K_DWG, "MI355_DWG", NOKEY, 1, P_ON},                                          // dense filter gradient, storing form: whole 128 x 128 tiles of dW per block over all rows (dwg_tile.hpp)
    {K_DWG_NST, "MI355_DWG_NST", NOKEY, 3, P_DWG_NST},                             // dwg tiles: LDS stages (3 | 4)
    {K_RWCONV_DBG, "MI355_RWCONV_DBG", NOKEY, 0, P_INT},                           // TIMING variants of the deconv3-forward register-weight instantiation: 1 no stores, 2 no LDS reads, 3 no MFMAs
    {K_RWCONV_WIDE, "MI355_RWCONV_WIDE", NOKEY, 1, P_ON},                          // 0: the 128 -> 64 channel layers stay on tapconv
    {K_LATENT_SPLIT, "MI355_LATENT_SPLIT", NOKEY, 16, P_RANGE, S_NONE, 1, 32},     // at most n K slices in the latent layers' split-K sums.  16 since late round 5 (32 before): half the slab traffic between the tall-K kernels and the reparameterisation
                                                                                   // kernels that sum them, one block per CU instead of two; step 0.8225 -> 0.8179 / 0.8153 -> 0.8125 ms on two boxes (12: the same, 8 and 24: slower)
    {K_DEBUG_GUARDS, "MI355_DEBUG_GUARDS", NOKEY, 0, P_OFF_PER_CALL},              // 256 guard bytes behind every workspace region; read whenever a workspace is sized or carved
    {K_RELU_BITS, "MI355_RELU_BITS", NOKEY, 1, P_ON},                              // 0: the input gradients read the activation tensors as ReluGrad masks
    {K_ARES, "MI355_ARES", NOKEY, 1, P_ON},                                        // activation-resident kernels (ares_tile.hpp): the engine carves by it, mi_ares_conv launches by it; 0: the general tile kernels
    {K_BWD_STREAMS, "MI355_BWD_STREAMS", NOKEY, 1, P_ON},                          // VAE backward: filter gradients on a second stream; 0 serialises everything
    {K_SLAB_BF16, "MI355_SLAB_BF16", NOKEY, 1, P_ON},                              // the bf16 VAE ENGINE rounds the partial-sum slabs of its backward pass to bf16 (0.966 -> 0.943 ms per step); 0: fp32 slabs.  Not key 18
    {K_DP_OPEN_JOIN, "MI355_DP_OPEN_JOIN", NOKEY, 1, P_ON},                        // data-parallel step: parts 0 and 1 leave the filter-gradient stream unjoined; 0: the joins of round 5
    {K_ARES_CFG, "MI355_ARES_CFG", NOKEY, 0, P_INT},                               // bit 0 conv form with 2 frames per block (two blocks per CU), bit 1 gather form with 8 (one block per CU)
    {K_ARES_DBG, "MI355_ARES_DBG", NOKEY, 0, P_INT},                               // TIMING mask of the activation-resident kernels
    {K_ARES_MID, "MI355_ARES_MID", NOKEY, 1, P_ON},                                // 0: the mid layers stay on the register-weight kernels
    {K_REPARAM_WIDE, "MI355_REPARAM_WIDE", NOKEY, 0, P_OFF},                       // the reparameterisation kernels request up to 32 slabs per element at once
    {K_PPO_PAD, "MI355_PPO_PAD", NOKEY, 0, P_RANGE, S_NONE, 0, 64},                // boundary-cost probe: empty launches between the PPO step's kernels (read only by builds with -DMI355_PPO_PAD_PROBE)
    {K_ENC12, "MI355_ENC12", NOKEY, 1, P_ON},                                      // fused encoder head (conv1 + conv2 in one launch, enc12_tile.hpp); the engine sizes its workspace by it
    {K_ENC12_RING, "MI355_ENC12_RING", NOKEY, 1, P_ON},                            // fused encoder head on camera bytes: the ring form of the conv1 stage's frame loads; 0: the compiler-scheduled form
    {K_ENC12_C2, "MI355_ENC12_C2", NOKEY, 1, P_ON},                                // fused encoder head on camera bytes: conv2's LDS fragment reads pipelined by hand; 0: the compiler-scheduled form
    {K_ENCHEAD, "MI355_ENCHEAD", NOKEY, 1, P_ON},                                  // fused encoder-head backward (enchead_tile.hpp)
    {K_PPO_FUSED, "MI355_PPO_FUSED", NOKEY, 1, P_ON},                              // fused PPO step; 0: the first-generation step (one launch per layer op)
    {K_PPO_STREAMS, "MI355_PPO_STREAMS", NOKEY, 0, P_OFF},                         // PPO backward on two streams: step 181 -> 172 us, but host cost per step 90 -> 135 us (3.25 -> 3.6 ms per update of 16 steps): off
    {K_MLP_STREAMS, "MI355_MLP_STREAMS", NOKEY, 1, P_ON},                          // MlpVAE full pass on two streams; 0: one stream
};
constexpr bool rows_in_enum_order() { for (int i = 0; i < K_COUNT; ++i) if (rows[i].id != i || (rows[i].key != NOKEY && rows[i].key != i)) return false; return true; }
static_assert(rows_in_enum_order(), "tuning.hip: row i must describe enumerator i, and a keyed knob's enumerator is its key");

int parse_env(const Row& r) {
    const char* e = r.env ? getenv(r.env) : nullptr;
    switch (r.parse) {
    case P_ON: return (e && e[0] == '0') ? 0 : 1;
    case P_OFF: case P_OFF_PER_CALL: return (e && e[0] == '1') ? 1 : 0;
    case P_INT: return e ? atoi(e) : r.def;
    case P_RANGE: { const int v = e ? atoi(e) : r.def; return v < r.lo || v > r.hi ? r.def : v; }
    case P_DWG_NST: return (e && atoi(e) == 4) ? 4 : 3;
    default: return r.def;
    }
}

// constructor priority 101: before every ordinary static initialiser of the library, whatever the order of its translation units
__attribute__((constructor(101))) void fill_from_environment() {
    for (int i = 0; i < K_COUNT; ++i) knob_values[i] = parse_env(rows[i]);
    if (!knob_values[K_TAPCONV]) knob_values[K_TAPCONV_MINBLOCKS] = -1;
}

}  // namespace

int knob_values[K_COUNT];

int knob_env_now(Knob k) { return parse_env(rows[k]); }

int knob_set(Knob k, int v) {
    const Row& r = rows[k];
    const int prev = knob_values[k];
    if (r.set == S_BOOL) v = v ? 1 : 0;
    else if (r.set == S_CLAMP) v = v < r.lo ? r.lo : v > r.hi ? r.hi : v;
    else if (r.set == S_DEF_OUTSIDE && (v < r.lo || v > r.hi)) v = r.def;
    if (r.set != S_IGNORED) knob_values[k] = v;
    return prev;
}

}  // namespace mi

extern "C" int mi_set_tuning(int key, int value) {
    if (key < 0 || key >= mi::K_COUNT || mi::rows[key].key != key) return mi_fail(MI_ERR_ARG, "mi_set_tuning: unknown key");
    return mi::knob_set((mi::Knob)key, value);
}
