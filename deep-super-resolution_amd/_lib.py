"""ctypes binding of csrc/libdsr_hip.so (C ABI: include/dsr_hip.h).

The HIP library is the product: there is NO fallback.  If the shared object is missing
or a symbol cannot be resolved this module raises, and every op that reaches `lib()` on a
machine without a GPU fails loudly.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
SO_PATH = os.path.join(_HERE, "csrc", "libdsr_hip.so")

ABI_VERSION = 9          # bumped whenever a signature in include/dsr_hip.h changes; checked against the loaded library
BF16, F16 = 0, 1
F32 = 2                  # the luma entry points (csrc/luma.hip) also read fp32 images
ACT_NONE, ACT_LEAKY, ACT_PRELU, ACT_RELU, ACT_TANH, ACT_SIGMOID, ACT_ELU = range(7)
PAD_ZERO, PAD_REFLECT, PAD_REPLICATE = range(3)
FEAT_L1, FEAT_MSE = 0, 1  # modes of the feature-loss taps (csrc/featloss.hip)
GRAM_LOSS_PARTIALS = 64   # doubles of scratch per image that dsr_gram_loss takes (DSR_GRAM_LOSS_PARTIALS, csrc/featstyle.hip)
GAN_VANILLA, GAN_LSGAN, GAN_HINGE = range(3)   # kinds of dsr_gan_loss (csrc/pointwise.hip)


class ConvDesc(C.Structure):
    _fields_ = [(n, C.c_int) for n in
                ("dtype", "N", "H", "W", "Cin", "Cout", "KH", "KW", "stride", "pad", "pad_mode")]


class Epilogue(C.Structure):
    _fields_ = [("act", C.c_int), ("slope", C.c_float), ("prelu", C.c_void_p), ("bias", C.c_void_p),
                ("stats_partial", C.c_void_p), ("pixel_shuffle", C.c_int), ("out_nchw_f32", C.c_void_p),
                ("bn_scale", C.c_void_p), ("bn_shift", C.c_void_p), ("residual", C.c_void_p)]


class RdbConv(C.Structure):
    """dsr_rdb_conv: one prefix convolution over a growth buffer (csrc/conv_rdb.hip)."""
    _fields_ = [("dtype", C.c_int), ("N", C.c_int), ("H", C.c_int), ("W", C.c_int), ("Cin", C.c_int), ("Cout", C.c_int),
                ("x", C.c_void_p), ("ldx", C.c_int), ("w", C.c_void_p), ("bias", C.c_void_p), ("act", C.c_int),
                ("slope", C.c_float), ("res1", C.c_void_p), ("ldr1", C.c_int), ("r1_off", C.c_int), ("beta1", C.c_float),
                ("res2", C.c_void_p), ("ldr2", C.c_int), ("r2_off", C.c_int), ("beta2", C.c_float), ("y", C.c_void_p),
                ("ldy", C.c_int), ("y_off", C.c_int), ("max_blocks", C.c_int)]


class RdbDgrad(C.Structure):
    """dsr_rdb_dgrad: one input gradient on a dense block's growth buffers (csrc/conv_rdb.hip)."""
    _fields_ = [("dtype", C.c_int), ("N", C.c_int), ("H", C.c_int), ("W", C.c_int), ("K", C.c_int), ("Cout", C.c_int),
                ("dy", C.c_void_p), ("lddy", C.c_int), ("dy_off", C.c_int), ("wd", C.c_void_p), ("scale", C.c_float),
                ("dx", C.c_void_p), ("lddx", C.c_int), ("accumulate", C.c_int), ("g", C.c_void_p), ("ldg", C.c_int),
                ("g_limit", C.c_int), ("g_scale", C.c_float), ("act_out", C.c_void_p), ("ldact", C.c_int),
                ("mask_lo", C.c_int), ("slope", C.c_float), ("max_blocks", C.c_int)]


class RdbWgrad(C.Structure):
    """dsr_rdb_wgrad: the ten parameter gradients of one dense block (csrc/conv_rdb_bwd.hip)."""
    _fields_ = [("dtype", C.c_int), ("N", C.c_int), ("H", C.c_int), ("W", C.c_int), ("x", C.c_void_p), ("ldx", C.c_int),
                ("dy", C.c_void_p), ("lddy", C.c_int), ("g", C.c_void_p), ("ldg", C.c_int), ("gscale", C.c_float),
                ("dw", C.c_void_p * 5), ("db", C.c_void_p * 5)]


class CompactConv(C.Structure):
    """dsr_compact_conv: one body layer of SRVGGNetCompact, conv + per-channel PReLU (csrc/conv_compact.hip)."""
    _fields_ = [("dtype", C.c_int), ("N", C.c_int), ("H", C.c_int), ("W", C.c_int), ("x", C.c_void_p), ("w", C.c_void_p),
                ("bias", C.c_void_p), ("slope", C.c_void_p), ("y", C.c_void_p), ("max_blocks", C.c_int)]


class CompactTail(C.Structure):
    """dsr_compact_tail: SRVGGNetCompact's tail, conv + PixelShuffle(s) + the input image (csrc/conv_compact.hip)."""
    _fields_ = [("dtype", C.c_int), ("N", C.c_int), ("H", C.c_int), ("W", C.c_int), ("C", C.c_int), ("s", C.c_int),
                ("x", C.c_void_p), ("w", C.c_void_p), ("bias", C.c_void_p), ("base", C.c_void_p), ("out", C.c_void_p),
                ("max_blocks", C.c_int)]


class AdamArgs(C.Structure):
    """dsr_adam_args: where an Adam launch takes its coefficients from (hyper, loss_scale, found_inf: device words, each
    nullable); one block for dsr_pw_adam, dsr_pw_adam_multi and dsr_linear_wgrad_adam."""
    _fields_ = [("step", C.c_void_p), ("lr", C.c_float), ("b1", C.c_float), ("b2", C.c_float), ("eps", C.c_float),
                ("grad_scale", C.c_float), ("hyper", C.c_void_p), ("loss_scale", C.c_void_p), ("found_inf", C.c_void_p)]


_P, _I, _F, _Z, _LL = C.c_void_p, C.c_int, C.c_float, C.c_size_t, C.c_longlong
_DESC = C.POINTER(ConvDesc)

# name -> (restype, argtypes); every symbol declared in include/dsr_hip.h
SIGNATURES = {
    "dsr_last_error": (C.c_char_p, []),
    "dsr_abi_version": (_I, []),
    "dsr_conv_dgrad_masked_supported": (_I, [_DESC]),
    "dsr_conv_dgrad_masked": (_I, [_DESC, _P, _P, _P, _I, _F, _P, _P]),
    "dsr_conv_dgrad_add_supported": (_I, [_DESC]),
    "dsr_conv_dgrad_add": (_I, [_DESC, _P, _P, _P, _P, _P]),
    "dsr_conv_wgrad_batchable": (_I, [_DESC]),
    "dsr_conv_wgrad_batched_workspace": (_Z, [_I, _DESC, C.POINTER(C.c_void_p)]),
    "dsr_conv_wgrad_batched": (_I, [_I, _DESC, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), _P, _Z, _P]),
    "dsr_conv_kernel_name": (C.c_char_p, [_DESC, _I, C.POINTER(Epilogue)]),
    "dsr_clock_sample": (_I, [_P, _P]),
    "dsr_resample_u8": (_I, [_P, _P, _I, _I, _I, _I, _I, _P, _P, _I, _P]),
    "dsr_noise_gaussian_u8": (_I, [_P, _P, _I, _P, _Z, _P]),
    "dsr_salt_pepper_u8": (_I, [_P, _P, _P, _P, _I, _I, _I, _P]),
    "dsr_scale_images_f32": (_I, [_P, _Z, _I, _P]),
    "dsr_patch_batch_u8": (_I, [_I, C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int),
                                C.POINTER(C.c_int), _I, _I, _I, _P, _P]),
    "dsr_patch_batch_u8_d4": (_I, [_I, C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int),
                                   C.POINTER(C.c_int), C.POINTER(C.c_int), _I, _I, _I, _P, _P]),
    "dsr_degrade_batch_u8": (_I, [_I, C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int),
                                  C.POINTER(C.c_int), C.POINTER(C.c_int), _I, _I, _I, _I, _P, _I, _P, _P, _I, _I, _P, _P]),
    "dsr_degrade_image_u8": (_I, [_P, _I, _I, _I, _I, _P, _I, _P, _P, _P, _P]),
    "dsr_jpeg_workspace": (_Z, [_I, _I, _I, _I]),
    "dsr_jpeg_u8": (_I, [_P, _P, _I, _I, _I, _P, _I, _P, _P]),
    "dsr_jpeg_batch_f32": (_I, [_P, _P, _I, _I, _I, _P, _I, _I, _P, _P]),
    "dsr_d4_expand_f32": (_I, [_P, _I, _I, _I, _I, _P, _P, _P]),
    "dsr_d4_mean_f32": (_I, [_P, _P, _I, _I, _I, _I, _P, _P]),
    "dsr_conv_fwd_affine_supported": (_I, [_DESC]),
    "dsr_conv_first_bwd_supported": (_I, [_DESC, _I]),
    "dsr_conv_first_bwd_workspace": (_Z, [_DESC]),
    "dsr_conv_first_bwd": (_I, [_DESC, _P, _P, _P, _I, _F, _P, _P, _P, _Z, _P]),
    "dsr_conv_first2_supported": (_I, [_DESC, _DESC]),
    "dsr_conv_first2_stats_rows": (_I, [_DESC]),
    "dsr_conv_first2_fwd": (_I, [_DESC, _DESC, _P, _P, _P, _F, _P, _P, _P, _P, _P, _P]),
    "dsr_conv_first_bwd_recompute": (_I, [_DESC, _P, _P, _P, _P, _I, _F, _P, _P, _P, _Z, _P]),
    "dsr_conv_dgrad_ps_supported": (_I, [_DESC]),
    "dsr_conv_dgrad_ps_rows": (_I, [_DESC]),
    "dsr_conv_dgrad_ps": (_I, [_DESC, _P, _P, _P, _P, _P, _P, _P]),
    "dsr_conv_dgrad_bn_supported": (_I, [_DESC]),
    "dsr_conv_dgrad_bn_rows": (_I, [_DESC]),
    "dsr_conv_dgrad_bn": (_I, [_DESC, _P, _P, _P, _P, _P, _P, _I, _F, _P, _P]),
    "dsr_conv_dgrad_first_bwd_supported": (_I, [_DESC, _DESC, _I]),
    "dsr_conv_dgrad_first_bwd_workspace": (_Z, [_DESC]),
    "dsr_conv_dgrad_first_bwd": (_I, [_DESC, _DESC, _P, _P, _P, _P, _P, _I, _F, _P, _P, _P, _Z, _P]),
    "dsr_conv_out_size": (_I, [_DESC, C.POINTER(_I), C.POINTER(_I)]),
    "dsr_conv_stats_rows": (_I, [_DESC]),
    "dsr_conv_packed_elems": (_Z, [_DESC, _I]),
    "dsr_conv_pack_weight": (_I, [_DESC, _P, _P, _P, _P]),
    "dsr_conv_pack_weight_multi": (_I, [_I, _I, _P, _P, _P, _P, _P, _P, _P]),
    "dsr_conv_fwd": (_I, [_DESC, _P, _P, C.POINTER(Epilogue), _P, _P]),
    "dsr_conv_dgrad_workspace": (_Z, [_DESC]),
    "dsr_conv_dgrad": (_I, [_DESC, _P, _P, _P, _P, _Z, _P]),
    "dsr_conv_wgrad_workspace": (_Z, [_DESC]),
    "dsr_conv_wgrad": (_I, [_DESC, _P, _P, _P, _P, _Z, _P]),
    "dsr_pw_nchw_to_nhwc": (_I, [_I, _P, _P, _I, _I, _I, _I, _I, _P]),
    "dsr_pw_nhwc_to_nchw": (_I, [_I, _P, _P, _I, _I, _I, _I, _I, _P]),
    "dsr_pw_pack_weight": (_I, [_I, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P]),
    "dsr_pw_scratch_rows": (_I, []),
    "dsr_pw_sum_rows": (_I, [_P, _I, _I, _I, _I, _F, _P, _I, _I, _P]),
    "dsr_pw_bn_finalize": (_I, [_P, _I, _I, _I, _I, _F, _P, _P, _P, _P, _P, _F, _F, _I, _P, _P, _P, _P, _P]),
    "dsr_pw_bn_eval_affine": (_I, [_P, _P, _P, _P, _F, _I, _I, _P, _P, _P, _P, _P]),
    "dsr_pw_reduce_blocks": (_I, [_Z, C.POINTER(_I)]),
    "dsr_pw_channel_stats": (_I, [_I, _P, _Z, _I, _I, _I, _P, _P]),
    "dsr_pw_bn_act_fwd": (_I, [_I, _P, _P, _P, _P, _P, _Z, _I, _I, _F, _P, _P]),
    "dsr_pw_bn_act_bwd_reduce": (_I, [_I, _P, _P, _P, _P, _P, _P, _Z, _I, _I, _I, _I, _F, _P, _P, _P]),
    "dsr_pw_bn_bwd_finalize": (_I, [_P, _I, _I, _I, _F, _P, _P, _P, _P, _P, _P, _P, _P]),
    "dsr_pw_bn_act_bwd_apply": (_I, [_I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _Z, _I, _I, _F, _P, _I, _P]),
    "dsr_pw_act_bwd": (_I, [_I, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _F, _P, _I, _I, _P, _P]),
    "dsr_pw_act_bwd_nchw": (_I, [_I, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P]),
    "dsr_pw_colsum": (_I, [_I, _P, _Z, _I, _I, _I, _P, _P]),
    "dsr_pw_add": (_I, [_I, _P, _P, _P, _Z, _P]),
    "dsr_pw_axpby_f32": (_I, [_P, _P, _F, _F, _P, _P, _Z, _P]),
    "dsr_pw_diff_loss": (_I, [_P, _P, _P, _Z, _I, _P, _I, _P]),
    "dsr_pw_bce_const": (_I, [_P, _I, _F, _P, _P, _I, _P]),
    "dsr_pw_adam": (_I, [_P, _P, _P, _P, _Z, _P, C.POINTER(AdamArgs), _P]),
    "dsr_pw_adam_multi": (_I, [_I, _P, _P, _P, _P, _P, C.POINTER(AdamArgs), _P]),
    "dsr_pw_incr": (_I, [_P, _P, _P]),
    "dsr_amp_check": (_I, [_I, C.POINTER(C.c_void_p), C.POINTER(_Z), _P, _P]),
    "dsr_amp_update": (_I, [_P, _P, _P, _F, _F, _I, _P, _P]),
    "dsr_clip_sumsq_partials": (_Z, [_I, C.POINTER(C.c_void_p), C.POINTER(_Z)]),
    "dsr_clip_sumsq": (_I, [_I, C.POINTER(C.c_void_p), C.POINTER(_Z), _P, _Z, _P]),
    "dsr_clip_finalize": (_I, [_P, _I, _P, _I, _F, _P, _F, _P, _F, _P, _P, _P, _P]),
    "dsr_cast16": (_I, [_I, _P, _P, _Z, _P]),
    "dsr_flatten": (_I, [_I, _P, _P, _I, _I, _I, _I, _I, _I, _P]),
    "dsr_linear_fwd_workspace": (_Z, [_I, _Z, _I]),
    "dsr_linear_fwd": (_I, [_I, _P, _P, _P, _I, _F, _P, _I, _Z, _I, _P, _Z, _P]),
    "dsr_linear_dgrad": (_I, [_I, _P, _P, _P, _I, _I, _Z, _P]),
    "dsr_linear_wgrad": (_I, [_I, _P, _P, _P, _I, _I, _Z, _P]),
    "dsr_linear_wgrad_gathered": (_I, [_I, _P, _P, _P, _I, _I, _Z, _I, _F, _P]),
    "dsr_linear_wgrad_adam": (_I, [_I, _P, _P, _I, _I, _Z, _I, _F, _P, _P, _P, _P, C.POINTER(AdamArgs), _P]),
    "dsr_linear_factor_gram_workspace": (_Z, [_I, _I, _Z, _I]),
    "dsr_linear_factor_gram_dots": (_I, [_I, _I]),
    "dsr_linear_factor_gram": (_I, [_I, _P, _P, _I, _I, _Z, _I, _F, _P, _Z, _P]),
    "dsr_dense2_fwd": (_I, [_P, _P, _P, _I, _I, _P, _P]),
    "dsr_dense2_bwd": (_I, [_I, _P, _P, _P, _P, _I, _I, _I, _F, _P, _P, _P, _P, _P, _P]),
    "dsr_maxpool2_fwd": (_I, [_I, _P, _P, _I, _I, _I, _I, _P]),
    "dsr_maxpool2_bwd": (_I, [_I, _P, _P, _P, _I, _I, _I, _I, _P]),
    "dsr_maxpool2_relu_bwd": (_I, [_I, _P, _P, _P, _I, _I, _I, _I, _P]),
    "dsr_avgpool2_fwd": (_I, [_I, _P, _P, _I, _I, _I, _I, _P]),
    "dsr_avgpool2_bwd": (_I, [_I, _P, _P, _I, _I, _I, _I, _P]),
    "dsr_nearest2x_fwd": (_I, [_I, _P, _P, _I, _I, _I, _I, _P]),
    "dsr_nearest2x_bwd": (_I, [_I, _P, _P, _I, _I, _I, _I, _P]),
    "dsr_bilinear2x_fwd": (_I, [_I, _P, _P, _I, _I, _I, _I, _P]),
    "dsr_bilinear2x_bwd": (_I, [_I, _P, _P, _I, _I, _I, _I, _P]),
    "dsr_resize_norm_fwd": (_I, [_I, _P, _P, _I, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _I, _P, _P, _P]),
    "dsr_resize_norm_bwd": (_I, [_I, _P, _P, _I, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _I, _P, _P]),
    "dsr_box_copy": (_I, [_P, _P] + [_I] * 16 + [_P]),
    "dsr_downsample_fwd": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _I, _P]),
    "dsr_downsample_bwd": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _I, _P]),
    "dsr_downsample_dense_fwd": (_I, [_P, _P, _P, _P] + [_I] * 7 + [_P]),
    "dsr_downsample_dense_dgrad": (_I, [_P, _P, _P] + [_I] * 7 + [_P]),
    "dsr_downsample_dense_wgrad_workspace": (_Z, [_I] * 7),
    "dsr_downsample_dense_wgrad": (_I, [_P, _P, _P, _P, _P, _Z] + [_I] * 7 + [_P]),
    "dsr_lpips_tap_sizes": (_I, [_I, _I, C.POINTER(_I)]),
    "dsr_lpips_stem_prep": (_I, [_I, _P, _P, _I, _I, _I, _I, _P, _P, _P]),
    "dsr_maxpool3s2_fwd": (_I, [_I, _P, _P, _I, _I, _I, _I, _P]),
    "dsr_lpips_distance_blocks": (_I, [_I, C.POINTER(_I), _I]),
    "dsr_lpips_distance": (_I, [_I, _I, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(_I), C.POINTER(_I),
                                C.POINTER(_I), _I, _P, _P]),
    "dsr_lpips_finalize": (_I, [_I, C.POINTER(_I), _I, _P, _P, _P, _F, _I, _P]),
    "dsr_lpips_distance_bwd": (_I, [_I, _I, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(_I), C.POINTER(_I),
                                    C.POINTER(_I), _I, _P, _F, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), _P]),
    "dsr_maxpool3s2_bwd": (_I, [_I, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P]),
    "dsr_lpips_stem_prep_bwd": (_I, [_I, _P, _I, _I, _I, _I, _F, _P, _P]),
    "dsr_ssim_img_blocks": (_I, [_I, _I, _I, _I]),
    "dsr_ssim_img_f32": (_I, [_P, _P, _I, _I, _I, _I, _F, _F, _P, _P, _P, _F, _I, _P]),
    "dsr_ssim_bwd_f32": (_I, [_P, _P, _I, _I, _I, _I, _F, _F, _P, _P, _P, _P]),
    "dsr_msssim_min_size": (_I, [_I]),
    "dsr_msssim_pyramid_floats": (_Z, [_I, _I, _I, _I, _I]),
    "dsr_ssim_cs_img_blocks": (_I, [_I, _I, _I, _I]),
    "dsr_ssim_cs_img_f32": (_I, [_P, _P, _I, _I, _I, _I, _F, _F, _P, _P, _P, _P]),
    "dsr_avgpool2_pair_f32": (_I, [_P, _P, _P, _P, _I, _I, _I, _P]),
    "dsr_msssim_combine": (_I, [_P, _I, _I, C.POINTER(_F), _I, _P, _P, _P, _F, _P, _P]),
    "dsr_msssim_bwd_blocks": (_I, [_I, _I, _I, _I]),
    "dsr_msssim_bwd_f32": (_I, [_P, _P, _I, _I, _I, _I, _F, _F, _P, _P, _P, _P, _P, _P, _P, _P]),
    "dsr_psnr_blocks": (_I, [_I, _I]),
    "dsr_psnr_stats_f32": (_I, [_P, _P, _I, _I, _P, _P, _P]),
    "dsr_psnr_finalize": (_I, [_P, _P, _I, _I, _I, _F, _F, _P, _P, _F, _P, _P]),
    "dsr_metric_accumulate": (_I, [_P, _I, _P, _P]),
    "dsr_metric_compute": (_I, [_P, _I, _I, _F, _F, _P, _P]),
    "dsr_lbfgs_workspace": (_Z, [_I, _Z, _I]),
    "dsr_lbfgs_vector_floats": (_Z, [_I, _Z]),
    "dsr_lbfgs_gather": (_I, [_I, C.POINTER(C.c_void_p), C.POINTER(_Z), _P, _Z, _P, _I, _Z, _P]),
    "dsr_lbfgs_dots": (_I, [_P, _Z, _P, _I, _Z, _I, _P]),
    "dsr_lbfgs_scalar": (_I, [_P, _Z, _I, _Z, _I, _P, _I, _P, C.c_double, _I, _I, C.c_double, C.c_double, _P]),
    "dsr_lbfgs_combine": (_I, [_I, C.POINTER(C.c_void_p), C.POINTER(_Z), _P, _Z, _P, _I, _Z, _P]),
    "dsr_ema_update_multi": (_I, [_I, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(_Z), C.POINTER(C.c_ubyte), _F, _I,
                                  _P, _P, _P]),
    "dsr_ema_tick": (_I, [_P, _P, _P]),
    "dsr_ema_swap_multi": (_I, [_I, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(_Z), _P]),
    "dsr_luma_blocks": (_I, [_I, _I, _I, _I]),
    "dsr_luma_sse_stats": (_I, [_I, _P, _I, _P, _I, _I, _I, _I, _I, _I, _P, _P]),
    "dsr_luma_pair": (_I, [_I, _P, _I, _P, _I, _I, _I, _I, _I, _I, _P, _P, _P, _P]),
    "dsr_rgb_to_y": (_I, [_I, _P, _I, _I, _I, _I, _I, _I, _P, _P]),
    "dsr_luma_psnr_finalize": (_I, [_P, _I, _I, _I, _I, _P, _P, _F, _P, _P]),
    "dsr_featloss_blocks": (_I, [_Z]),
    "dsr_featloss_tap_fwd": (_I, [_I, _P, _P, _P, _Z, _I, _I, _P, _P]),
    "dsr_featloss_fold": (_I, [_P, _I, _F, _P, _P]),
    "dsr_featloss_tap_bwd": (_I, [_I, _P, _P, _P, _P, _F, _I, _I, _P, _Z, _I, _P]),
    "dsr_featloss_relu": (_I, [_I, _P, _P, _Z, _I, _P]),
    "dsr_featloss_combine": (_I, [_I, C.POINTER(C.c_void_p), C.POINTER(_F), _P, _P]),
    "dsr_featloss_combine_bwd": (_I, [_I, C.POINTER(_F), _P, _P, _P]),
    "dsr_gram_chunks": (_I, [_I]),
    "dsr_gram_workspace": (_Z, [_I, _I, _I]),
    "dsr_gram_fwd": (_I, [_I, _P, _I, _I, _I, _I, _F, _P, _P, _P]),
    "dsr_gram_loss": (_I, [_I, _P, _P, _I, _I, _I, _I, _P, _P, _P, _P, _P]),
    "dsr_featstyle_tap_bwd": (_I, [_I, _P, _P, _P, _P, _F, _I, _I, _P, _P, _P, _F, _P, _I, _I, _I, _P]),
    "dsr_imresize_f32": (_I, [_P, _P, _I, _I, _I, _I, _I, _P, _P, _I, _P, _P, _I, _P]),
    "dsr_imresize_u8": (_I, [_P, _P, _I, _I, _I, _I, _I, _P, _P, _I, _P, _P, _I, _P]),
    "dsr_conv_rdb_supported": (_I, [C.POINTER(RdbConv)]),
    "dsr_conv_rdb_fwd": (_I, [C.POINTER(RdbConv), _P]),
    "dsr_conv_rdb_dgrad_supported": (_I, [C.POINTER(RdbDgrad)]),
    "dsr_conv_rdb_dgrad": (_I, [C.POINTER(RdbDgrad), _P]),
    "dsr_conv_rdb_wgrad_supported": (_I, [C.POINTER(RdbWgrad)]),
    "dsr_conv_rdb_wgrad_workspace": (_Z, [C.POINTER(RdbWgrad)]),
    "dsr_conv_rdb_wgrad_chunks": (_I, [C.POINTER(RdbWgrad)]),
    "dsr_conv_rdb_wgrad": (_I, [C.POINTER(RdbWgrad), _P, _Z, _P]),
    "dsr_scale_add16": (_I, [_I, _P, _F, _P, _P, _Z, _P]),
    "dsr_spectral_norm_workspace": (_Z, [_I, C.POINTER(_I), C.POINTER(_I)]),
    "dsr_spectral_norm_bwd_workspace": (_Z, [_I, C.POINTER(_I), C.POINTER(_I)]),
    "dsr_spectral_norm_fwd": (_I, [_I, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(_I),
                                   C.POINTER(_I), _I, _F, _P, C.POINTER(C.c_void_p), _P, _Z, _P]),
    "dsr_spectral_norm_bwd": (_I, [_I, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                                   C.POINTER(_I), C.POINTER(_I), _P, C.POINTER(C.c_void_p), _P, _Z, _P]),
    "dsr_gan_loss_blocks": (_I, [_Z]),
    "dsr_gan_loss": (_I, [_P, _Z, _I, _I, _I, _P, _P, _P, _P]),
    "dsr_rel_gan_loss_workspace": (_Z, [_Z, _Z]),
    "dsr_rel_gan_loss": (_I, [_P, _Z, _P, _Z, _I, _I, _I, _P, _P, _P, _P, _P]),
    "dsr_ldl_workspace": (_Z, [_I, _I, _I, _I, _I]),
    "dsr_ldl_fwd": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _P, _P, _P, _P]),
    "dsr_ldl_bwd": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P, _P]),
    "dsr_filter2d_f32": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _I, _P]),
    "dsr_noise_gaussian_f32": (_I, [_P, _P, _P, _P, _P, _P, _I, _I, _I, _P]),
    "dsr_noise_poisson_f32": (_I, [_P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _P]),
    "dsr_usm_mask": (_I, [_P, _P, _F, _P, _Z, _P]),
    "dsr_usm_combine": (_I, [_P, _P, _P, _F, _P, _Z, _P]),
    "dsr_niqe_plane": (_I, [_I, _P, _I, _I, _I, _I, _I, _P, _P]),
    "dsr_niqe_moments": (_I, [_P, _I, _I, _I, _I, _P, _P, _P]),
    "dsr_niqe_features": (_I, [_P, _P, _I, _I, _P, _P, _P]),
    "dsr_conv_prelu_c_supported": (_I, [C.POINTER(CompactConv)]),
    "dsr_conv_prelu_c_fwd": (_I, [C.POINTER(CompactConv), _P]),
    "dsr_conv_shuffle_add_supported": (_I, [C.POINTER(CompactTail)]),
    "dsr_conv_shuffle_add_fwd": (_I, [C.POINTER(CompactTail), _P]),
    "dsr_pw_prelu_c_fwd": (_I, [_I, _P, _P, _P, _Z, _I, _I, _P]),
    "dsr_pw_prelu_c_rows": (_I, [_Z]),
    "dsr_pw_prelu_c_fold_width": (_I, []),
    "dsr_pw_prelu_c_bwd": (_I, [_I, _P, _P, _P, _P, _Z, _I, _I, _P, _P, _P]),
    "dsr_shuffle_add_f32": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _P]),
    "dsr_shuffle_add_bwd_f32": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _P]),
}

_lib = None

# bench.py's roofline leg: a list here makes every launching entry point record (name, start_event, end_event) on the
# stream it launches on (torch's current stream), so that the GPU-busy share of a step can be told from launch gaps.
LAUNCH_LOG = None
_NO_LAUNCH = ("dsr_last_error", "dsr_abi_version", "dsr_conv_dgrad_ps_supported", "dsr_conv_dgrad_ps_rows", "dsr_conv_dgrad_bn_supported", "dsr_conv_dgrad_bn_rows", "dsr_conv_dgrad_first_bwd_supported", "dsr_conv_dgrad_first_bwd_workspace", "dsr_conv_kernel_name", "dsr_conv_wgrad_batchable", "dsr_conv_wgrad_batched_workspace", "dsr_conv_dgrad_add_supported", "dsr_conv_dgrad_masked_supported", "dsr_conv_fwd_affine_supported",
              "dsr_conv_first2_supported", "dsr_conv_first2_stats_rows", "dsr_conv_first_bwd_supported", "dsr_conv_first_bwd_workspace", "dsr_conv_out_size", "dsr_conv_stats_rows",
              "dsr_conv_packed_elems", "dsr_conv_dgrad_workspace", "dsr_conv_wgrad_workspace", "dsr_pw_scratch_rows",
              "dsr_pw_reduce_blocks", "dsr_linear_fwd_workspace", "dsr_lpips_tap_sizes", "dsr_lpips_distance_blocks",
              "dsr_ssim_img_blocks", "dsr_psnr_blocks", "dsr_lbfgs_workspace", "dsr_lbfgs_vector_floats", "dsr_clip_sumsq_partials",
              "dsr_linear_factor_gram_workspace", "dsr_linear_factor_gram_dots", "dsr_downsample_dense_wgrad_workspace",
              "dsr_msssim_min_size", "dsr_msssim_pyramid_floats", "dsr_ssim_cs_img_blocks", "dsr_msssim_bwd_blocks", "dsr_luma_blocks",
              "dsr_featloss_blocks", "dsr_jpeg_workspace", "dsr_conv_rdb_supported", "dsr_conv_rdb_dgrad_supported",
              "dsr_conv_rdb_wgrad_supported", "dsr_conv_rdb_wgrad_workspace", "dsr_conv_rdb_wgrad_chunks", "dsr_spectral_norm_workspace",
              "dsr_spectral_norm_bwd_workspace", "dsr_gan_loss_blocks", "dsr_gram_chunks", "dsr_gram_workspace", "dsr_rel_gan_loss_workspace",
              "dsr_ldl_workspace", "dsr_conv_prelu_c_supported", "dsr_conv_shuffle_add_supported", "dsr_pw_prelu_c_rows",
              "dsr_pw_prelu_c_fold_width")


class _Lib:
    """The loaded shared object; attribute access returns the bound C function (optionally timed, see LAUNCH_LOG)."""

    def __init__(self, handle):
        self._h = handle
        for name in SIGNATURES:
            fn = getattr(handle, name)
            setattr(self, name, fn if name in _NO_LAUNCH else self._timed(name, fn))

    @staticmethod
    def _timed(name, fn):
        def call(*args):
            log = LAUNCH_LOG
            if log is None:
                return fn(*args)
            import torch
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            rc = fn(*args)
            e1.record()
            log.append((name, e0, e1))
            return rc
        return call


def lib():
    """The loaded library; raises if it was not built (run __graft_entry__.build())."""
    global _lib
    if _lib is None:
        if not os.path.exists(SO_PATH):
            raise RuntimeError(f"{SO_PATH} is missing: the HIP extension is the only implementation of this "
                               "package (no CPU fallback). Build it with `python -c 'import __graft_entry__ as g; g.build()'`.")
        h = C.CDLL(SO_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(h, name)          # AttributeError if the symbol is not exported
            fn.restype = res
            fn.argtypes = args
        got = h.dsr_abi_version()
        if got != ABI_VERSION:
            # a stale libdsr_hip.so under a newer binding (or the reverse) passes arguments in the wrong slots: the
            # kernels then read sizes as pointers -- refuse to run instead (round-1 bring-up abort)
            raise RuntimeError(f"{SO_PATH}: C-ABI version {got}, this binding expects {ABI_VERSION}; rebuild with "
                               "`python -c 'import __graft_entry__ as g; g.build()'`")
        _lib = _Lib(h)
    return _lib


def check(rc):
    if rc != 0:
        raise RuntimeError("dsr_hip: " + lib().dsr_last_error().decode())
    return rc


def _ptr(t):
    """One tensor's device pointer as a C argument; None stays None (a NULL argument)."""
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    """torch's current stream on the current device, as the C argument every launching entry point takes."""
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def ptr_table(tensors):
    """HOST table of device pointers for the multi-tensor entry points, one per tensor; None becomes a NULL entry."""
    return (C.c_void_p * len(tensors))(*[None if t is None else t.data_ptr() for t in tensors])


def size_table(values):
    """HOST table of size_t (element counts) for the multi-tensor entry points."""
    return (C.c_size_t * len(values))(*values)
