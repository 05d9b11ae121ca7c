// The C ABI of libstcat_hip.so, declared once: STCAT_ENTRY_POINTS(X) has one line X(name, "kinds") per exported function
// of include/stcat_hip.h, except the five that describe the ABI itself (stcat_version, stcat_last_error,
// stcat_entry_count / _name / _kinds).  Besides the prototype in the header and the definition, this list is the only
// place that names an entry point: the library's self-description (stcat_entry_*, what the Python side binds from) and
// the launch-plan table (stcat_capi.hip) are generated from it.
//
// kinds: one letter per argument —
//   p device pointer     P host pointer     s stream (void*, always last)     S C string
//   i int                l long             f float                           u unsigned long long
// Every line is checked against the function's own C type below, so a wrong letter does not compile.
#pragma once

#include "../../include/stcat_hip.h"
#include "launch_plan.h"

#define STCAT_ENTRY_POINTS(X) \
  X(stcat_frozen_bn_fold, "ppppppifs") \
  X(stcat_stem_fwd, "pppppiiis") \
  X(stcat_stem_u8_fwd, "pppppppiiis") \
  X(stcat_clip_resize, "piiiiiiiiiiiiiiiippps") \
  X(stcat_maxpool3x3s2, "ppiiiis") \
  X(stcat_conv_fwd, "ppppppiiiiiiiiiis") \
  X(stcat_conv_dgrad, "pppppppppiiiiiiiiis") \
  X(stcat_weight_transpose, "ppiiis") \
  X(stcat_weight_transpose_multi, "piis") \
  X(stcat_weight_transpose_entry_bytes, "") \
  X(stcat_conv_wgrad, "pppiiiiiiiiis") \
  X(stcat_act_bwd, "pppppliis") \
  X(stcat_pos_sine_2d, "pppiiis") \
  X(stcat_sine_embed_fwd, "pppis") \
  X(stcat_sine_embed_bwd, "ppppis") \
  X(stcat_linear_fwd, "pppppiiiiiiiils") \
  X(stcat_linear_dgrad, "pppppiiiiis") \
  X(stcat_linear_fwd_acc, "pppppiiiiiis") \
  X(stcat_linear_dgrad_acc, "ppppiiiiis") \
  X(stcat_linear_fwd_multi, "ippppppppppppppppppppppppppppppppiiis") \
  X(stcat_linear_dgrad_multi, "ippppppppppppppppppppppppppppppppiiis") \
  X(stcat_linear_wgrad_multi, "ippppppppppppppppppppppppppppppppiiis") \
  X(stcat_linear_fwd_drop, "pppppiiiiiiifllps") \
  X(stcat_linear_dgrad_mask, "pppppfpiiiiis") \
  X(stcat_linear_wgrad, "ppppiiiiis") \
  X(stcat_small_linear_fwd, "ppppiiis") \
  X(stcat_small_linear_bwd, "ppppppiiis") \
  X(stcat_colsum, "pppiis") \
  X(stcat_layernorm_fwd, "pppppppiiffllps") \
  X(stcat_layernorm_bwd, "ppppppppppiifllps") \
  X(stcat_ew, "ippppllffs") \
  X(stcat_ew2d, "iplplplliffs") \
  X(stcat_embed_ln_fwd, "ppppppppppiiiiffllps") \
  X(stcat_embed_ln_bwd, "pppppppppppppppiiiiifllps") \
  X(stcat_mha_d64_fwd, "ppppppiiiiiiiffllps") \
  X(stcat_mha_d64_bwd, "pppppppppiiiiiiiiiffllps") \
  X(stcat_stg_loss_fwd, "pppppppppppppfiiiiippps") \
  X(stcat_stg_loss_bwd, "pppppppppppppfiiiiippppppps") \
  X(stcat_dropout, "ppplfllps") \
  X(stcat_mha_self_fwd, "ppppppiiiiiiiffllps") \
  X(stcat_mha_self_bwd, "ppppppppppppiiiiiiiiiffllps") \
  X(stcat_mha_self_fwd_lse, "ppppppiiiiiiiffllps") \
  X(stcat_mha_self_bwd_lse, "ppppppppppiiiiiiiiiffllps") \
  X(stcat_mha_bs_fwd, "ppppppiiiiiiiffllps") \
  X(stcat_mha_bs_bwd, "ppppppppppiiiiiiiiiffllps") \
  X(stcat_attn_weights_mean, "ppiiifllps") \
  X(stcat_attn_q1_fwd, "ppppppppiiiiiiffllps") \
  X(stcat_attn_q1_bwd, "ppppppppppppiiiiiiffllps") \
  X(stcat_map2d_pool, "ppiiiis") \
  X(stcat_map2d_cells, "pppipiiis") \
  X(stcat_map2d_cells_bwd, "pppippiiis") \
  X(stcat_map2d_pool_bwd, "pppiiiis") \
  X(stcat_map2d_cells_bwd_gather, "pppipppiiis") \
  X(stcat_map2d_pool_bwd_gather, "pppiiiis") \
  X(stcat_rowscale, "ppliis") \
  X(stcat_pl_rowscale, "pppliis") \
  X(stcat_rank_sum, "ppillfs") \
  X(stcat_rank_tree_sum, "ppillfs") \
  X(stcat_grad_sqnorm, "pppiips") \
  X(stcat_grad_sqnorm_ws, "pppiippls") \
  X(stcat_adamw_ema_step, "pppiipPPifffiffs") \
  X(stcat_grad_accumulate, "pppiiifs") \
  X(stcat_grad_tree_fold, "pppiiiifs") \
  X(stcat_grad_clip_scale, "pppiipfs") \
  X(stcat_ema_update, "pppiifs") \
  X(stcat_optim_table_entry_bytes, "") \
  X(stcat_temporal_map_argmax, "pppiis") \
  X(stcat_pl_conv_fwd, "ppppppppppppiiiiiiiiiis") \
  X(stcat_pl_conv_dgrad, "pppppppppppppppiiiiiiiiis") \
  X(stcat_pl_linear_fwd, "ppppppppppiiiifllps") \
  X(stcat_pl_linear_dgrad_mask, "pppppppppiiis") \
  X(stcat_pl_colsum, "pppiis") \
  X(stcat_pl_split_sum, "pppppls") \
  X(stcat_pl_conv_dgrad_cadd, "ppppppippppiiiiis") \
  X(stcat_pl_conv_wgrad, "ppppppiiiiiiiiis") \
  X(stcat_pl_conv_wgrad_ws, "ppppppiiiiiiiiipls") \
  X(stcat_pl_maxpool3x3s2, "pppiiiis") \
  X(stcat_pl_split, "pppls") \
  X(stcat_pl_join, "pppls") \
  X(stcat_pl_act_bwd, "pppppppliis") \
  X(stcat_pl_scale, "ppppplis") \
  X(stcat_weight_planes_entry_bytes, "") \
  X(stcat_weight_planes_multi, "piis") \
  X(stcat_debug_force_pl_tile, "i") \
  X(stcat_debug_pl_flags, "i") \
  X(stcat_debug_force_tile, "ii") \
  X(stcat_debug_streamk, "i") \
  X(stcat_spin, "is") \
  X(stcat_stream_create, "iiP") \
  X(stcat_stream_destroy, "P") \
  X(stcat_set_mma_mode, "i") \
  X(stcat_get_mma_mode, "") \
  X(stcat_set_deterministic, "i") \
  X(stcat_get_deterministic, "") \
  X(stcat_set_f16_scales, "ii") \
  X(stcat_get_f16_scale, "i") \
  X(stcat_plan_fn_index, "S") \
  X(stcat_plan_fn_nargs, "i") \
  X(stcat_plan_create, "") \
  X(stcat_plan_destroy, "P") \
  X(stcat_plan_add_call, "PiPiii") \
  X(stcat_plan_add_wait, "Pii") \
  X(stcat_plan_add_memset, "Ppuii") \
  X(stcat_plan_set_word, "Piu") \
  X(stcat_plan_add_yield, "Pi") \
  X(stcat_plan_add_reloc, "Piiu") \
  X(stcat_plan_size, "PPPP") \
  X(stcat_plan_run, "PPiPiiPP")

#define STCAT_CHECK_KINDS(name, kinds)                                                                                \
  static_assert(stcat_plan::kinds_match<decltype(&name)>(kinds, stcat_plan::same_str(#name, "stcat_plan_create")), \
                #name ": kinds do not match its C type");
STCAT_ENTRY_POINTS(STCAT_CHECK_KINDS)
#undef STCAT_CHECK_KINDS

// the check itself: stcat_ew is (int, const float*, const float*, const float*, float*, long, long, float, float, void*)
static_assert(!stcat_plan::kinds_match<decltype(&stcat_ew)>("ippppilffs"), "a long is not an i");
static_assert(!stcat_plan::kinds_match<decltype(&stcat_ew)>("ippppllfs"), "one letter short");
static_assert(!stcat_plan::kinds_match<decltype(&stcat_ew)>("ippppllfsf"), "the stream comes last");
// (stcat_pl_rowscale's first argument is a void*: only its position keeps it from being an s)
static_assert(!stcat_plan::kinds_match<decltype(&stcat_pl_rowscale)>("sppliis"), "the stream comes last");
static_assert(!stcat_plan::kinds_match<decltype(&stcat_ew)>("ippppllffs", true), "returns int, not a handle");
