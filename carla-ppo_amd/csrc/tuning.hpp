// tuning.hpp — every tuning knob of the library, declared once: the rows (environment name, mi_set_tuning key, default, parse rule, clamp, what it selects) are the
// table in tuning.hip.  The table is filled from the environment once, when the library is loaded and before any other static initialiser of it runs; a launcher
// reads a knob with mi::knob(K_...): one array load, no lock, no string.  Thread-local per-pass state (the slab / reduce deferral modes) is not knob state.
#pragma once

namespace mi {

enum Knob : int {     // K_0 .. K_26 in key order: the enumerator of a keyed knob IS its mi_set_tuning key (static_assert in tuning.hip); then the environment-only knobs by file
    K_GEMM2, K_TAPCONV_MINBLOCKS, K_WGRAD_DBG, K_TAPWGRAD, K_NARROW, K_TAP_VARIANT, K_TAP_DIRECT, K_TAPWGRAD_SPLIT, K_KEY8_REMOVED, K_TAPWGRAD_BLOCKS,
    K_NW_BLOCK_WAVES, K_DENSE_WGRAD_BLOCKS, K_TAP_MASK_PREFETCH, K_RWCONV, K_TAPWGRAD_CW, K_RWCONV_CONV, K_RWCONV_BLOCKS, K_GEMM2_TILE, K_SLAB_BF16_DEFAULT,
    K_NW_DEPTH, K_GEMM2_STAGES, K_X3_TAPWGRAD, K_DWGS, K_ENC12_DBG, K_TW_LDEC, K_DECTAIL_DBG, K_DECTAIL_SPLIT5,
    K_TAPCONV, K_GEMM2_SPLITK, K_GEMM2_REMAP3, K_REDUCE_RY_CAP, K_NARROW_LEAN, K_NW_WAVES, K_TALLK, K_DECTAIL, K_DECTAIL_EDGE, K_DWG, K_DWG_NST,      // conv_ops.hip
    K_RWCONV_DBG, K_RWCONV_WIDE,                                                                                                                // rwconv.hip
    K_LATENT_SPLIT, K_DEBUG_GUARDS, K_RELU_BITS, K_ARES, K_BWD_STREAMS, K_SLAB_BF16, K_DP_OPEN_JOIN,                                          // vae_engine.hip (K_ARES, K_DECTAIL: and their launchers)
    K_ARES_CFG, K_ARES_DBG, K_ARES_MID, K_REPARAM_WIDE, K_PPO_PAD, K_ENC12, K_ENC12_RING, K_ENC12_C2, K_ENCHEAD, K_PPO_FUSED, K_PPO_STREAMS, K_MLP_STREAMS,
    K_COUNT
};

extern int knob_values[K_COUNT];
inline int knob(Knob k) { return knob_values[k]; }
int knob_set(Knob k, int v);      // applies the row's mi_set_tuning clamp; returns the previous value
int knob_env_now(Knob k);         // parses the row's environment string NOW (the rows marked per-call: K_DEBUG_GUARDS); the table value is not touched

}  // namespace mi
