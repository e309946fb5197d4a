"""ctypes binding of libecgmm_hip.so (C ABI declared in include/ecgmm.h).

The library is the product: there is NO CPU or eager-PyTorch fallback.  Importing this module never
touches the GPU; the first call of :func:`lib` loads the shared object and fails loudly when it is
missing (build it with ``python __graft_entry__.py`` or ``make -C ecg-multimodal-model_amd/csrc``).
"""
import ctypes as C
import os

F32, BF16 = 0, 1
ACT_NONE, ACT_RELU, ACT_SIGMOID = 0, 1, 2
RESNET18_NPARAMS, RESNET18_NBUFFERS = 62, 60
RESNET1D_NPARAMS, RESNET1D_NBUFFERS = 52, 27

_PKG_DIR = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# ECGMM_LIB: A/B another build of the same library (kernel experiments); default = the in-tree build
LIB_PATH = os.environ.get("ECGMM_LIB") or os.path.join(_PKG_DIR, "libecgmm_hip.so")

vp, i32, i64, u64, f32, f64, sz = C.c_void_p, C.c_int, C.c_int64, C.c_uint64, C.c_float, C.c_double, C.c_size_t


class ConvDesc(C.Structure):
    _fields_ = [(n, i32) for n in ("N", "H", "W", "Cin", "Cout", "R", "S", "stride", "pad_h", "pad_w")]


class ResNet18Desc(C.Structure):
    _fields_ = [("N", i32), ("H", i32), ("W", i32), ("out_dim", i32), ("dtype", i32), ("training", i32),
                ("bn_momentum", f32), ("bn_eps", f32)]


class ResNet1DDesc(C.Structure):
    _fields_ = [("N", i32), ("cin", i32), ("L", i32), ("num_classes", i32), ("dtype", i32), ("training", i32),
                ("bn_momentum", f32), ("bn_eps", f32), ("dropout_p", f32), ("seed", u64), ("offset", u64)]


class HeadDesc(C.Structure):
    _fields_ = [("B", i32), ("dim", i32 * 3), ("hidden", i32), ("num_classes", i32), ("training", i32),
                ("ln_eps", f32), ("dropout_p", f32), ("seed", u64), ("offset", u64)]


class LSTMDesc(C.Structure):
    _fields_ = [(n, i32) for n in ("B", "T", "In", "H", "layers", "bidirectional", "batch_first", "save_for_backward")]


class MHADesc(C.Structure):
    _fields_ = [(n, i32) for n in ("S", "N", "heads", "head_dim", "batch_first")] + [("p_drop", f32)]


class CRNNFrontDesc(C.Structure):
    _fields_ = [("B", i32), ("F", i32), ("T", i32), ("dtype", i32), ("training", i32), ("bn_momentum", f32), ("bn_eps", f32)]


class TransformerInferDesc(C.Structure):
    _fields_ = [(n, i32) for n in ("B", "L", "input_dim", "E", "heads", "ff", "layers", "classes", "batch_first")] + [("eps", f32)]


class TabNetInferDesc(C.Structure):
    _fields_ = [(n, i32) for n in ("input_dim", "n_d", "n_a", "n_steps", "n_shared", "n_independent", "out_dim")] + \
               [("gamma", f32), ("epsilon", f32), ("bn_eps", f32)]


P = C.POINTER
# name -> (restype, argtypes).  Must list every function declared in include/ecgmm.h
# (tests/test_abi.py parses the header and checks the two agree).
SIGNATURES = {
    "ecgmm_version": (i32, []),
    "ecgmm_last_error": (C.c_char_p, []),
    "ecgmm_switch_name": (C.c_char_p, [i32]),
    "ecgmm_switch_get": (i32, [C.c_char_p, P(i64)]),
    "ecgmm_switch_set": (i32, [C.c_char_p, i64]),
    "ecgmm_resnet18_fwd_workspace": (sz, [P(ResNet18Desc)]),
    "ecgmm_resnet18_bwd_workspace": (sz, [P(ResNet18Desc)]),
    "ecgmm_resnet18_forward": (i32, [P(ResNet18Desc), vp, P(vp), P(vp), vp, vp, sz, vp]),
    "ecgmm_resnet18_backward": (i32, [P(ResNet18Desc), vp, vp, P(vp), P(vp), vp, vp, sz, i32, i32, vp]),
    "ecgmm_resnet18_backward_dx": (i32, [P(ResNet18Desc), vp, vp, P(vp), P(vp), vp, vp, sz, i32, i32, vp, vp]),
    "ecgmm_resnet18_gradcam": (i32, [P(ResNet18Desc), vp, P(vp), vp, vp, sz, vp, vp]),
    "ecgmm_resnet18_ws_view": (i32, [P(ResNet18Desc), i32, C.c_char_p, i32, P(sz), P(sz)]),
    "ecgmm_head_fwd_workspace": (sz, [P(HeadDesc)]),
    "ecgmm_head_bwd_workspace": (sz, [P(HeadDesc)]),
    "ecgmm_head_forward": (i32, [P(HeadDesc), P(vp), P(vp), P(vp), vp, vp, vp, sz, vp]),
    "ecgmm_head_backward": (i32, [P(HeadDesc), P(vp), P(vp), P(vp), P(vp), vp, P(vp), vp, vp, sz, vp]),
    "ecgmm_conv_halo_enable": (i32, [i32]),
    "ecgmm_conv_halo_cus": (i32, [i32]),
    "ecgmm_conv_halo_w4": (i32, [i32]),
    "ecgmm_conv_halo_stagger": (i32, [i32]),
    "ecgmm_conv_halo_stream": (i32, [i32]),
    "ecgmm_conv_halo_pingpong": (i32, [i32]),
    "ecgmm_conv_wgrad_pingpong": (i32, [i32]),
    "ecgmm_conv_wgrad_ring_enable": (i32, [i32]),
    "ecgmm_side_wgrad": (i32, [i32]),
    "ecgmm_side_defer_join": (i32, [i32]),
    "ecgmm_resnet1d_side_wgrad": (i32, [i32]),
    "ecgmm_side_wait": (i32, [vp]),
    "ecgmm_side_stream": (vp, []),
    "ecgmm_side_fork": (i32, [vp]),
    "ecgmm_resnet1d_fwd_workspace": (sz, [P(ResNet1DDesc)]),
    "ecgmm_resnet1d_bwd_workspace": (sz, [P(ResNet1DDesc)]),
    "ecgmm_resnet1d_forward": (i32, [P(ResNet1DDesc), vp, P(vp), P(vp), vp, vp, sz, vp]),
    "ecgmm_resnet1d_backward": (i32, [P(ResNet1DDesc), vp, vp, P(vp), P(vp), vp, vp, sz, i32, i32, vp]),
    "ecgmm_resnet1d_backward_dx": (i32, [P(ResNet1DDesc), vp, vp, P(vp), P(vp), vp, vp, sz, i32, i32, vp, vp]),
    "ecgmm_resnet1d_gradcam": (i32, [P(ResNet1DDesc), vp, P(vp), vp, vp, sz, vp, vp]),
    "ecgmm_resnet1d_ws_view": (i32, [P(ResNet1DDesc), i32, C.c_char_p, i32, P(sz), P(sz)]),
    "ecgmm_nchw_to_nhwc": (i32, [i32, vp, vp, i32, i32, i64, vp]),
    "ecgmm_nhwc_to_nchw": (i32, [i32, vp, vp, i32, i32, i64, vp]),
    "ecgmm_cast": (i32, [i32, vp, vp, i64, vp]),
    "ecgmm_uncast": (i32, [i32, vp, vp, i64, vp]),
    "ecgmm_pack_conv_weight": (i32, [i32, vp, vp, vp, i32, i32, i32, vp]),
    "ecgmm_conv_stats_rows": (i32, [i64]),
    "ecgmm_conv_fwd": (i32, [i32, P(ConvDesc), vp, vp, vp, vp, vp, i32, vp]),
    "ecgmm_conv_fwd_wgrows": (i32, [i32, P(ConvDesc), vp, vp, vp, vp, vp, vp, i32, vp]),
    "ecgmm_conv_bwd_data": (i32, [i32, P(ConvDesc), vp, vp, vp, vp, vp]),
    "ecgmm_conv_bwd_weight_workspace": (sz, [i32, P(ConvDesc)]),
    "ecgmm_conv_bwd_weight": (i32, [i32, P(ConvDesc), vp, vp, vp, i32, vp, sz, vp]),
    "ecgmm_stem_packed_elems": (sz, [i32, i32]),
    "ecgmm_stem_stats_rows": (i32, [i32, i32, i32, i32, i32]),
    "ecgmm_stem_pack": (i32, [i32, vp, vp, i32, i32, vp]),
    "ecgmm_stem_fwd": (i32, [i32, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, vp]),
    "ecgmm_stem_wg_stats_rows": (i32, [i32, i32, i32, i32, i32]),
    "ecgmm_stem_fwd_wgrows": (i32, [i32, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, vp]),
    "ecgmm_stem_stats_only_rows": (i32, [i32, i32, i32, i32, i32]),
    "ecgmm_stem_stats_only": (i32, [i32, vp, vp, vp, vp, i32, i32, i32, i32, i32, vp]),
    "ecgmm_stem_pool_fwd": (i32, [vp, vp, vp, vp, vp, i32, i32, i32, i32, vp]),
    "ecgmm_stem_pool_bwd_workspace": (sz, [i32, i32, i32, i32]),
    "ecgmm_stem_pool_bwd": (i32, [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, sz, i32, i32, i32, i32, vp]),
    "ecgmm_stem_bwd_weight_workspace": (sz, [i32, i32, i32, i32, i32]),
    "ecgmm_stem_bwd_weight": (i32, [i32, vp, vp, vp, i32, vp, sz, i32, i32, i32, i32, i32, vp]),
    "ecgmm_stem_bwd_data": (i32, [i32, vp, vp, vp, i32, i32, i32, i32, i32, vp]),
    "ecgmm_col_stats_rows": (i32, [i32, i64, i32]),
    "ecgmm_col_stats": (i32, [i32, vp, i64, i32, vp, vp]),
    "ecgmm_bn_finalize": (i32, [vp, i32, i32, f64, vp, vp, vp, vp, vp, f32, f32, vp, vp]),
    "ecgmm_bn_eval_coef": (i32, [i32, vp, vp, vp, vp, f32, vp, vp]),
    "ecgmm_bn_act": (i32, [i32, vp, vp, vp, vp, vp, i32, i32, vp, i64, i32, vp]),
    "ecgmm_bn_act_from_rows": (i32, [i32, vp, vp, i32, f64, vp, vp, vp, vp, vp, f32, f32, vp, vp, vp, vp, i32, i32, vp, i64, i32, vp]),
    "ecgmm_bn_bwd_scratch": (sz, [i32, i64, i32]),
    "ecgmm_bn_bwd": (i32, [i32, vp, vp, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, i64, i32, vp, vp]),
    "ecgmm_bn_eval_bwd": (i32, [i32, vp, vp, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp, i64, i32, vp, vp]),
    "ecgmm_conv_bwd_data_with_downsample": (i32, [i32, P(ConvDesc), vp, vp, vp, vp, vp, vp, vp]),
    "ecgmm_conv_bwd_data_bnred": (i32, [i32, P(ConvDesc), vp, vp, vp, vp, vp, vp, vp, vp, P(i32), vp]),
    "ecgmm_conv_bwd_data_bnred_rows": (i32, [i32, P(ConvDesc)]),
    "ecgmm_bn_bwd_from_rows": (i32, [i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, i64, i32, vp, vp]),
    "ecgmm_bnrelu_maxpool": (i32, [i32, vp, vp, vp, vp, i32, i32, i32, i32, vp]),
    "ecgmm_maxpool_relu_bwd": (i32, [i32, vp, vp, vp, vp, i32, i32, i32, i32, vp]),
    "ecgmm_bn_fuse_min_pixels": (i32, [i64]),
    "ecgmm_bn_fold": (i32, [i32]),
    "ecgmm_bn_fold_slice": (i32, [i32]),
    "ecgmm_bn_act_from_rows_bits": (i32, [i32, vp, vp, i32, f64, vp, vp, vp, vp, vp, f32, f32, vp, vp, vp, vp, i32, i32, vp, vp, i64, i32, vp]),
    "ecgmm_bn_bwd_bits": (i32, [i32, vp, vp, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, i64, i32, vp, vp]),
    "ecgmm_bn_bwd_dual": (i32, [i32] + [vp] * 19 + [i64, i32, vp, vp, vp]),
    "ecgmm_bn_dual": (i32, [i32]),
    "ecgmm_tl_enable": (i32, [i32]),
    "ecgmm_tl_mark": (i32, [i32, vp]),
    "ecgmm_tl_collect": (i32, [i32, vp, vp]),
    "ecgmm_stem_recompute": (i32, [i32]),
    "ecgmm_pool_bn_bwd": (i32, [i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, vp, vp]),
    "ecgmm_avgpool": (i32, [i32, vp, vp, i32, i32, i32, vp, vp]),
    "ecgmm_bcast_rows": (i32, [i32, vp, vp, i32, i32, i32, f32, vp]),
    "ecgmm_se_gate_grad": (i32, [i32, vp, vp, vp, vp, vp, i32, i32, i32, vp]),
    "ecgmm_se_gate_bn": (i32, [i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, vp]),
    "ecgmm_se_mlp_fwd": (i32, [vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, vp]),
    "ecgmm_se_mlp_bwd": (i32, [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, f32, vp]),
    "ecgmm_linear_fwd": (i32, [vp, vp, vp, vp, i32, i32, i32, i32, vp]),
    "ecgmm_linear_bwd_scratch": (sz, [i32, i32, i32]),
    "ecgmm_linear_bwd": (i32, [vp, vp, vp, vp, vp, vp, i32, i32, i32, vp, sz, vp]),
    "ecgmm_act_bwd": (i32, [vp, vp, vp, i64, i32, vp]),
    "ecgmm_layernorm_fwd": (i32, [P(vp), P(i32), i32, vp, vp, vp, vp, vp, vp, i32, f32, vp]),
    "ecgmm_layernorm_bwd_scratch": (sz, [i32, i32]),
    "ecgmm_layernorm_bwd": (i32, [P(vp), P(i32), i32, vp, vp, vp, vp, P(vp), i32, vp, vp, vp, i32, vp, vp]),
    "ecgmm_varloss_fwd": (i32, [vp, vp, vp, i32, i32, i32, i32, vp, vp, vp]),
    "ecgmm_varloss_bwd": (i32, [vp, i32, i32, vp, vp, i32, vp, i32, vp]),
    "ecgmm_ce_fwd": (i32, [vp, vp, i32, i32, i32, f32, f32, vp, vp, vp]),
    "ecgmm_ce_bwd": (i32, [vp, vp, i32, i32, vp, vp, vp, vp]),
    "ecgmm_ce_plus_fwd": (i32, [vp, vp, i32, i32, vp, f32, vp, vp, vp]),
    "ecgmm_ce_plus_bwd": (i32, [vp, vp, i32, i32, vp, vp, vp, vp, f32, vp]),
    "ecgmm_dropout_fwd": (i32, [vp, vp, vp, i64, f32, u64, u64, vp]),
    "ecgmm_dropout_bwd": (i32, [vp, vp, vp, i64, f32, vp]),
    "ecgmm_adam": (i32, [vp, vp, vp, vp, i64, f32, f32, f32, f32, f32, i64, f32, vp]),
    "ecgmm_axpby": (i32, [f32, vp, f32, vp, i64, vp]),
    "ecgmm_signal_preprocess_workspace": (sz, [i32, i32, i32]),
    "ecgmm_signal_preprocess": (i32, [vp, vp, i32, i32, vp, vp, i32, P(f64), P(f64), P(f64), i32, vp, sz, vp]),
    "ecgmm_signal_preprocess_i16": (i32, [vp, i32, i32, i32, P(i32), i32, vp, vp, i32, vp, i32, i32, P(f64), P(f64), P(f64),
                                          i32, vp]),
    "ecgmm_weighted_sample": (i32, [vp, i64, i64, vp, vp, i64, u64, u64, vp]),
    "ecgmm_signal_filter_zscore": (i32, [vp, vp, i32, i32, P(f64), P(f64), P(f64), i32, i32, f64, vp]),
    "ecgmm_signal_filter_lanes": (i32, [P(f64), i32, i32]),
    "ecgmm_signal_resample_len": (i32, [i32, f64]),
    "ecgmm_signal_resample_workspace": (sz, [i32, i32, i32]),
    "ecgmm_signal_resample": (i32, [vp, i32, i32, vp, i32, f64, vp, i32, vp, vp, sz, vp]),
    "ecgmm_signal_gather_augment": (i32, [vp, i64, i32, vp, i32, vp, vp, i32, f32, f32, f32, f32, i32, i32, u64, u64, vp]),
    "ecgmm_glu_fwd": (i32, [vp, vp, i64, i32, vp]),
    "ecgmm_glu_bwd": (i32, [vp, vp, vp, i64, i32, vp]),
    "ecgmm_sparsemax_fwd": (i32, [vp, vp, i64, i32, vp]),
    "ecgmm_sparsemax_bwd": (i32, [vp, vp, vp, i64, i32, vp]),
    "ecgmm_ew": (i32, [i32, vp, vp, vp, i64, f32, vp]),
    "ecgmm_split_cols": (i32, [vp, vp, vp, i64, i32, i32, i32, vp]),
    "ecgmm_split_cols_bwd": (i32, [vp, vp, vp, vp, i64, i32, i32, i32, vp]),
    "ecgmm_bn_small_fwd": (i32, [vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, f32, f32, vp]),
    "ecgmm_bn_small_bwd": (i32, [vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, vp]),
    "ecgmm_bn_small_eval_bwd": (i32, [vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, vp]),
    "ecgmm_entropy_fwd": (i32, [vp, vp, i64, i32, f32, vp]),
    "ecgmm_entropy_bwd": (i32, [vp, vp, vp, i64, i32, f32, vp]),
    "ecgmm_image_resize_tables_bytes": (sz, [i32, i32, i32, i32]),
    "ecgmm_image_resize_tables": (i32, [i32, i32, i32, i32, vp, sz]),
    "ecgmm_image_transform": (i32, [vp, vp, i32, i32, i32, i32, i32, vp, sz, P(f32), P(f32), vp]),
    "ecgmm_resnet18_infer_prepared_bytes": (sz, [P(ResNet18Desc)]),
    "ecgmm_resnet18_infer_prepare": (i32, [P(ResNet18Desc), P(vp), P(vp), vp, sz, vp]),
    "ecgmm_resnet18_infer_workspace": (sz, [P(ResNet18Desc)]),
    "ecgmm_resnet18_infer": (i32, [P(ResNet18Desc), vp, vp, sz, vp, vp, sz, vp]),
    "ecgmm_resnet1d_infer_prepared_bytes": (sz, [P(ResNet1DDesc)]),
    "ecgmm_resnet1d_infer_prepare": (i32, [P(ResNet1DDesc), P(vp), P(vp), vp, sz, vp]),
    "ecgmm_resnet1d_infer_workspace": (sz, [P(ResNet1DDesc)]),
    "ecgmm_resnet1d_infer": (i32, [P(ResNet1DDesc), vp, vp, sz, vp, vp, sz, vp]),
    "ecgmm_infer_down_side": (i32, [i32]),
    "ecgmm_conv_fwd_fused": (i32, [i32, P(ConvDesc), vp, vp, vp, vp, vp, i32, vp]),
    "ecgmm_fold_conv_bn": (i32, [i32, i32, vp, vp, vp, vp, vp, vp, f32, vp, vp, vp, i32, i32, i32, vp]),
    "ecgmm_relu_maxpool": (i32, [i32, vp, vp, i32, i32, i32, i32, vp]),
    "ecgmm_gate_res_relu": (i32, [i32, vp, vp, vp, vp, i64, i32, i32, vp]),
    "ecgmm_prof_enable": (i32, [i32]),
    "ecgmm_prof_pause": (i32, [i32]),
    "ecgmm_prof_collect": (i32, [i32, P(f64), P(f64), P(f64), P(i64)]),
    "ecgmm_lstm_fwd_workspace": (sz, [P(LSTMDesc)]),
    "ecgmm_lstm_bwd_workspace": (sz, [P(LSTMDesc)]),
    "ecgmm_lstm_forward": (i32, [P(LSTMDesc), vp, P(vp), vp, vp, vp, vp, vp, vp, sz, vp]),
    "ecgmm_lstm_backward": (i32, [P(LSTMDesc), vp, P(vp), vp, vp, vp, vp, vp, vp, vp, P(vp), vp, vp, vp, sz, vp]),
    "ecgmm_lstm_forward_varlen": (i32, [P(LSTMDesc), vp, vp, P(vp), vp, vp, vp, vp, vp, vp, sz, vp]),
    "ecgmm_lstm_backward_varlen": (i32, [P(LSTMDesc), vp, vp, P(vp), vp, vp, vp, vp, vp, vp, vp, P(vp), vp, vp, vp, sz,
                                         vp]),
    "ecgmm_lstm_fwd_workspace_dt": (sz, [P(LSTMDesc), i32]),
    "ecgmm_lstm_bwd_workspace_dt": (sz, [P(LSTMDesc), i32]),
    "ecgmm_lstm_forward_dt": (i32, [P(LSTMDesc), i32, vp, vp, P(vp), vp, vp, vp, vp, vp, vp, sz, vp]),
    "ecgmm_lstm_backward_dt": (i32, [P(LSTMDesc), i32, vp, vp, P(vp), vp, vp, vp, vp, vp, vp, vp, P(vp), vp, vp, vp, sz,
                                     vp]),
    "ecgmm_lstm_ws_view": (i32, [P(LSTMDesc), i32, C.c_char_p, i32, i32, P(sz), P(sz)]),
    "ecgmm_seq_mean_varlen_fwd": (i32, [vp, vp, vp, i32, i32, i32, vp]),
    "ecgmm_seq_mean_varlen_bwd": (i32, [vp, vp, vp, i32, i32, i32, vp]),
    "ecgmm_conv5_in1_stats_rows": (i32, [i32, i32, i32]),
    "ecgmm_conv5_in1_fwd": (i32, [i32, vp, vp, vp, vp, vp, i32, i32, i32, vp]),
    "ecgmm_conv5_in1_bwd_weight_workspace": (sz, [i32, i32, i32]),
    "ecgmm_conv5_in1_bwd_weight": (i32, [i32, vp, vp, vp, vp, i32, vp, sz, i32, i32, i32, vp]),
    "ecgmm_conv5_bwd_weight_workspace": (sz, [i32, P(ConvDesc)]),
    "ecgmm_conv5_bwd_weight": (i32, [i32, P(ConvDesc), vp, vp, vp, i32, vp, sz, vp]),
    "ecgmm_bnrelu_maxpool2": (i32, [i32, vp, vp, vp, vp, i32, i32, i32, i32, i32, vp]),
    "ecgmm_pool2_bn_bwd_workspace": (sz, [i32, i32, i32, i32]),
    "ecgmm_pool2_bn_bwd": (i32, [i32, vp, vp, vp, vp, i32, vp, vp, vp, vp, i32, i32, i32, i32, i32, vp, sz, vp]),
    "ecgmm_crnn_front_fwd_workspace": (sz, [P(CRNNFrontDesc)]),
    "ecgmm_crnn_front_bwd_workspace": (sz, [P(CRNNFrontDesc)]),
    "ecgmm_crnn_front_forward": (i32, [P(CRNNFrontDesc), vp, P(vp), P(vp), vp, vp, sz, vp]),
    "ecgmm_crnn_front_backward": (i32, [P(CRNNFrontDesc), vp, vp, P(vp), P(vp), vp, vp, sz, vp]),
    "ecgmm_crnn_front_backward_dx": (i32, [P(CRNNFrontDesc), vp, vp, P(vp), P(vp), vp, vp, sz, vp, vp]),
    "ecgmm_conv5_in1_bwd_data": (i32, [i32, vp, vp, vp, i32, i32, i32, vp]),
    "ecgmm_conv5_in1_bwd_data_tile": (None, [i32, P(i32), P(i32), P(i32)]),
    "ecgmm_crnn_gradcam_workspace": (sz, [i32, i32, i32, i32]),
    "ecgmm_crnn_gradcam": (i32, [vp, vp, vp, vp, vp, sz, vp, i32, i32, i32, i32, i32, i32, vp]),
    "ecgmm_gradcam": (i32, [i32, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, vp]),
    "ecgmm_relu_maxpool2": (i32, [i32, vp, vp, i32, i32, i32, i32, i32, vp]),
    "ecgmm_conv5_in1_relu_pool2": (i32, [i32, vp, vp, vp, vp, i32, i32, i32, vp]),
    "ecgmm_fold_conv5_bn": (i32, [i32, i32, vp, vp, vp, vp, vp, vp, f32, vp, vp, vp, i32, i32, vp]),
    "ecgmm_crnn_front_infer_prepared_bytes": (sz, [P(CRNNFrontDesc)]),
    "ecgmm_crnn_front_infer_prepare": (i32, [P(CRNNFrontDesc), P(vp), P(vp), vp, sz, vp]),
    "ecgmm_crnn_front_infer_workspace": (sz, [P(CRNNFrontDesc)]),
    "ecgmm_crnn_front_infer": (i32, [P(CRNNFrontDesc), vp, vp, sz, vp, vp, sz, vp]),
    "ecgmm_log_spectrogram_frames": (i32, [i32, i32, i32]),
    "ecgmm_log_spectrogram": (i32, [vp, i32, i32, vp, i32, i32, vp, i32, vp]),
    "ecgmm_lime_perturb": (i32, [vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, u64, u64, vp, vp, vp, vp, vp]),
    "ecgmm_lime_ridge_workspace": (sz, [i32, i32, i32]),
    "ecgmm_lime_ridge": (i32, [vp, vp, vp, vp, i32, i32, i32, i32, i32, f64, f64, vp, vp, vp, vp, vp, vp, sz, vp]),
    "ecgmm_lime_prob": (i32, [vp, i64, i32, i32, vp, i64, vp]),
    "ecgmm_shap_mlp_workspace": (sz, [i32, i32, i32, i32, i32]),
    "ecgmm_shap_gradient": (i32, [vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, vp, vp, vp, vp, sz, vp]),
    "ecgmm_shap_deep": (i32, [vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, vp, vp, vp, vp, sz, vp]),
    "ecgmm_mha_bwd_workspace": (sz, [P(MHADesc)]),
    "ecgmm_mha_forward": (i32, [P(MHADesc), vp, vp, vp, u64, u64, vp]),
    "ecgmm_mha_backward": (i32, [P(MHADesc), vp, vp, vp, vp, vp, vp, sz, u64, u64, vp]),
    "ecgmm_mha_keep_mask": (i32, [P(MHADesc), vp, u64, u64, vp]),
    "ecgmm_mha_forward_varlen": (i32, [P(MHADesc), vp, vp, vp, vp, u64, u64, vp]),
    "ecgmm_mha_backward_varlen": (i32, [P(MHADesc), vp, vp, vp, vp, vp, vp, vp, sz, u64, u64, vp]),
    "ecgmm_mha_weights": (i32, [P(MHADesc), vp, vp, vp, vp, i32, vp]),
    "ecgmm_mha_rollout_step": (i32, [P(MHADesc), vp, vp, vp, vp, vp, f32, vp]),
    "ecgmm_embed1d_fwd": (i32, [vp, vp, vp, vp, vp, i32, i32, i32, i32, vp]),
    "ecgmm_embed1d_bwd_workspace": (sz, [i32, i32, i32, i32]),
    "ecgmm_embed1d_bwd": (i32, [vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, vp, sz, vp]),
    "ecgmm_linear_res_ln": (i32, [vp, vp, vp, vp, vp, vp, vp, i64, i32, i32, f32, vp]),
    "ecgmm_ffn_res_ln": (i32, [vp, vp, vp, vp, vp, vp, vp, vp, i64, i32, i32, f32, vp]),
    "ecgmm_transformer_infer_prepared_bytes": (sz, [P(TransformerInferDesc)]),
    "ecgmm_transformer_infer_prepare": (i32, [P(TransformerInferDesc), P(vp), vp, sz, vp]),
    "ecgmm_transformer_infer_workspace": (sz, [P(TransformerInferDesc)]),
    "ecgmm_transformer_infer": (i32, [P(TransformerInferDesc), vp, vp, vp, sz, vp, vp, sz, vp]),
    "ecgmm_tabnet_infer_prepared_bytes": (sz, [P(TabNetInferDesc)]),
    "ecgmm_tabnet_infer_prepare": (i32, [P(TabNetInferDesc), P(vp), vp, sz, vp]),
    "ecgmm_tabnet_infer": (i32, [P(TabNetInferDesc), vp, i64, vp, sz, vp, vp, vp, vp, vp]),
}

# Entry points of the input-gradient / Grad-CAM feature.  A library selected with ECGMM_LIB for an A/B run may predate them:
# it still loads, and calling one of them then fails with a message instead of a missing attribute.
LATER_SYMBOLS = ("ecgmm_resnet18_backward_dx", "ecgmm_resnet18_gradcam", "ecgmm_resnet1d_backward_dx",
                 "ecgmm_resnet1d_gradcam", "ecgmm_stem_bwd_data", "ecgmm_bn_eval_bwd", "ecgmm_bn_small_eval_bwd",
                 # the inference plans (ecgmm/inference.py)
                 "ecgmm_resnet18_infer_prepared_bytes", "ecgmm_resnet18_infer_prepare", "ecgmm_resnet18_infer_workspace",
                 "ecgmm_resnet18_infer", "ecgmm_resnet1d_infer_prepared_bytes", "ecgmm_resnet1d_infer_prepare",
                 "ecgmm_resnet1d_infer_workspace", "ecgmm_resnet1d_infer", "ecgmm_infer_down_side", "ecgmm_conv_fwd_fused",
                 "ecgmm_fold_conv_bn", "ecgmm_relu_maxpool", "ecgmm_gate_res_relu",
                 # the PhysioNet-2017 path (ecgmm/train_physionet.py)
                 "ecgmm_signal_filter_zscore", "ecgmm_signal_gather_augment",
                 # nn.LSTM (ecgmm.hip.nn.LSTM)
                 "ecgmm_lstm_fwd_workspace", "ecgmm_lstm_bwd_workspace", "ecgmm_lstm_forward", "ecgmm_lstm_backward",
                 # the CRNN front end's per-op kernels (csrc/crnn_front.hip)
                 "ecgmm_conv5_in1_stats_rows", "ecgmm_conv5_in1_fwd", "ecgmm_conv5_in1_bwd_weight_workspace",
                 "ecgmm_conv5_in1_bwd_weight", "ecgmm_conv5_bwd_weight_workspace", "ecgmm_conv5_bwd_weight",
                 "ecgmm_bnrelu_maxpool2", "ecgmm_pool2_bn_bwd_workspace", "ecgmm_pool2_bn_bwd",
                 "ecgmm_crnn_front_fwd_workspace", "ecgmm_crnn_front_bwd_workspace", "ecgmm_crnn_front_forward",
                 "ecgmm_crnn_front_backward",
                 # the switch table by name (csrc/switches.h)
                 "ecgmm_switch_name", "ecgmm_switch_get", "ecgmm_switch_set",
                 # the log-spectrogram (ecgmm/spectrogram.py, csrc/spectrogram.hip)
                 "ecgmm_log_spectrogram_frames", "ecgmm_log_spectrogram",
                 # the SE MLP per-op (csrc/head_fused.hip)
                 "ecgmm_se_mlp_fwd", "ecgmm_se_mlp_bwd",
                 # the PTB-XL path (ecgmm/train_signal_only_ptb.py)
                 "ecgmm_signal_preprocess_i16", "ecgmm_weighted_sample",
                 # the workspace views of the two encoder plans (tests/test_plan_replay_*.py)
                 "ecgmm_resnet18_ws_view", "ecgmm_resnet1d_ws_view",
                 # LIME of the fusion head (ecgmm/lime_tabular.py, csrc/lime.hip)
                 "ecgmm_lime_perturb", "ecgmm_lime_ridge_workspace", "ecgmm_lime_ridge", "ecgmm_lime_prob",
                 # SHAP of the fusion head (ecgmm/shap_explainers.py, csrc/shap.hip)
                 "ecgmm_shap_mlp_workspace", "ecgmm_shap_gradient", "ecgmm_shap_deep",
                 # the dual BatchNorm backward of the downsample blocks (csrc/elementwise.hip)
                 "ecgmm_bn_bwd_dual", "ecgmm_bn_dual",
                 # the Transformer encoder (ecgmm.hip.nn.TransformerEncoder, csrc/attention.hip)
                 "ecgmm_mha_bwd_workspace", "ecgmm_mha_forward", "ecgmm_mha_backward", "ecgmm_mha_keep_mask",
                 "ecgmm_embed1d_fwd", "ecgmm_embed1d_bwd_workspace", "ecgmm_embed1d_bwd",
                 # the merged SE / BatchNorm backward's first pass, per op (csrc/elementwise.hip)
                 "ecgmm_se_gate_bn",
                 # variable-length sequences: lengths in the LSTM, the masked mean (csrc/lstm.hip)
                 "ecgmm_lstm_forward_varlen", "ecgmm_lstm_backward_varlen", "ecgmm_seq_mean_varlen_fwd",
                 "ecgmm_seq_mean_varlen_bwd",
                 # the lane rule of the chunked filtfilt kernels (csrc/preprocess.hip)
                 "ecgmm_signal_filter_lanes",
                 # lengths in the attention kernels (csrc/attention.hip)
                 "ecgmm_mha_forward_varlen", "ecgmm_mha_backward_varlen",
                 # attention maps and the rollout step (ecgmm.explain.attention_maps / attention_rollout)
                 "ecgmm_mha_weights", "ecgmm_mha_rollout_step",
                 # saliency of the spectrogram CRNN (ecgmm.explain.spectrogram_gradients / spectrogram_grad_cam)
                 "ecgmm_crnn_front_backward_dx", "ecgmm_conv5_in1_bwd_data", "ecgmm_conv5_in1_bwd_data_tile",
                 "ecgmm_crnn_gradcam_workspace", "ecgmm_crnn_gradcam",
                 # Fourier resampling (ecgmm.preprocess.resample, csrc/resample.hip)
                 "ecgmm_signal_resample_len", "ecgmm_signal_resample_workspace", "ecgmm_signal_resample",
                 # the CRNN front end's inference plan (ecgmm.inference.Predictor(CRNN), csrc/plan_infer.hip)
                 "ecgmm_relu_maxpool2", "ecgmm_conv5_in1_relu_pool2", "ecgmm_fold_conv5_bn",
                 "ecgmm_crnn_front_infer_prepared_bytes", "ecgmm_crnn_front_infer_prepare",
                 "ecgmm_crnn_front_infer_workspace", "ecgmm_crnn_front_infer",
                 # the transformer's fused layer tails and inference plan (ecgmm.inference.Predictor(ECGTransformer1D))
                 "ecgmm_linear_res_ln", "ecgmm_ffn_res_ln", "ecgmm_transformer_infer_prepared_bytes",
                 "ecgmm_transformer_infer_prepare", "ecgmm_transformer_infer_workspace", "ecgmm_transformer_infer",
                 # TabNet's fused eval forward and masks (ecgmm.inference._TabNetPlan, csrc/tabnet_infer.hip)
                 "ecgmm_tabnet_infer_prepared_bytes", "ecgmm_tabnet_infer_prepare", "ecgmm_tabnet_infer",
                 # the encoders' Grad-CAM map kernels on their own (csrc/gradcam.hip)
                 "ecgmm_gradcam",
                 # the LSTM recurrence in a compute dtype (ecgmm.hip.nn.LSTM(compute_dtype=...), csrc/lstm.hip)
                 "ecgmm_lstm_fwd_workspace_dt", "ecgmm_lstm_bwd_workspace_dt", "ecgmm_lstm_forward_dt",
                 "ecgmm_lstm_backward_dt", "ecgmm_lstm_ws_view")

_lib = None


def _missing(name):
    def fail(*_a):
        raise RuntimeError(f"{LIB_PATH} does not export {name}: rebuild the HIP library (there is no fallback)")
    return fail


def lib():
    """Load (once) and return the ctypes handle; raises if the HIP library is not built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"libecgmm_hip.so not found at {LIB_PATH}: the HIP extension is the only compute path "
                "(no CPU fallback). Build it with `python __graft_entry__.py` or "
                "`make -C ecg-multimodal-model_amd/csrc`.")
        # torch ships its own libamdhip64: import it first so that this library binds to the SAME HIP
        # runtime instance (two runtimes in one process do not see each other's device context)
        import torch  # noqa: F401
        h = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            if name in LATER_SYMBOLS and os.environ.get("ECGMM_LIB") and not hasattr(h, name):
                setattr(h, name, _missing(name))
                continue
            fn = getattr(h, name)
            fn.restype, fn.argtypes = res, args
        if h.ecgmm_version() != 100:
            raise RuntimeError(f"libecgmm_hip.so version {h.ecgmm_version()} != 100 (stale build?)")
        _lib = h
    return _lib


def check(rc, what=""):
    if rc != 0:
        msg = lib().ecgmm_last_error().decode(errors="replace")
        raise RuntimeError(f"ecgmm {what} failed (code {rc}): {msg}")
