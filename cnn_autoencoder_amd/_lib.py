"""ctypes binding of libcae_hip.so (C ABI declared in include/cae_hip.h).

There is no CPU fallback: if the library is missing or fails to load, importing the hot
path raises.  Build it with ``python -c "import __graft_entry__ as g; g.build()"`` or
``make -C cnn_autoencoder_amd/csrc``.
"""
from __future__ import annotations

import ctypes
import os
import subprocess
import threading

import torch  # noqa: F401  (loads torch's libamdhip64 first so both share one HIP runtime)

_HERE = os.path.dirname(os.path.abspath(__file__))
# CAE_LIB: alternative build of the same library (kernel A/B experiments); never a different implementation
LIB_PATH = os.environ.get('CAE_LIB') or os.path.join(_HERE, 'libcae_hip.so')
_lock = threading.Lock()
_lib = None

c_void_p = ctypes.c_void_p
c_int = ctypes.c_int
c_size_t = ctypes.c_size_t
c_float = ctypes.c_float

# every symbol include/cae_hip.h declares: name -> (restype, argtypes)
SYMBOLS = {
    'cae_version': (c_int, []),
    'cae_last_error': (ctypes.c_char_p, []),
    'cae_free': (None, [c_void_p]),
    'cae_model_create': (c_int, [c_int, c_int, c_int, c_int, c_int, ctypes.POINTER(c_void_p)]),
    'cae_model_destroy': (None, [c_void_p]),
    'cae_model_set_layer': (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    'cae_model_set_layer_act': (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p]),
    'cae_model_set_precision': (c_int, [c_void_p, c_int]),
    'cae_last_range_ticket': (ctypes.c_int64, []),
    'cae_range_check': (c_int, [c_void_p, ctypes.c_int64, c_void_p]),
    'cae_thread_force_fp32': (None, [c_int]),
    'cae_model_effective_precision': (c_int, [c_void_p, c_void_p]),
    'cae_model_set_entropy': (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    'cae_analysis': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    'cae_analysis_levels': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    'cae_synthesis': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_void_p]),
    'cae_model_set_layer_stage': (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int,
                                           c_int, c_int]),
    'cae_model_set_color_layer': (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p]),
    'cae_synthesis_multiscale': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_void_p,
                                          c_void_p]),
    'cae_analysis_symbols': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    'cae_synthesis_symbols': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_void_p]),
    'cae_synthesis_scale': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_int, c_void_p]),
    'cae_synthesis_symbols_scale': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_int, c_void_p]),
    'cae_gdn_forward': (c_int, [c_void_p, c_int, c_int, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p]),
    'cae_quantize': (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p]),
    'cae_quantize_export': (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_int, c_void_p]),
    'cae_copy_to_host': (c_int, [c_void_p, c_void_p, c_size_t]),
    'cae_dequantize': (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p]),
    'cae_model_set_density': (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_float]),
    'cae_model_set_likelihood_form': (c_int, [c_void_p, c_int]),
    'cae_likelihood': (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    'cae_tile_ssim': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_size_t, c_void_p]),
    'cae_tile_delta_e': (c_int, [c_void_p, c_void_p, c_int, c_size_t, c_void_p, c_void_p, c_size_t, c_void_p]),
    'cae_u8hwc_to_planes': (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    'cae_avgpool2': (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p]),
    'cae_msssim_level': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    'cae_tile_sse': (c_int, [c_void_p, c_void_p, c_int, c_size_t, c_void_p, c_void_p]),
    'cae_model_set_profiling': (c_int, [c_void_p, c_int]),
    'cae_model_get_profile': (c_int, [c_void_p, c_int, c_void_p, c_int, c_void_p, c_int]),
    'cae_t_packed_bytes': (c_size_t, [c_int, c_int, c_int]),
    'cae_t_pack_weights': (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    'cae_t_from_nchw': (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    'cae_t_to_nchw': (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    'cae_t_set_samples_per_block': (c_int, [c_int]),
    'cae_t_conv_forward': (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_void_p, c_int,
                                    c_void_p, c_void_p]),
    'cae_t_conv_dgrad_ext': (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_int, c_int, c_int, c_void_p, c_int,
                                      c_void_p]),
    'cae_t_deconv_forward': (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_void_p, c_int,
                                      c_void_p, c_void_p]),
    'cae_t_deconv_dgrad': (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_void_p, c_int,
                                    c_void_p]),
    'cae_t_wgrad': (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p,
                             c_void_p]),
    'cae_t_gdn_forward': (c_int, [c_void_p, ctypes.c_long, c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p]),
    'cae_t_gdn_backward': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p,
                                    c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    'cae_t_conv_forward_act': (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_void_p, c_int,
                                        c_void_p, c_int, c_void_p]),
    'cae_t_deconv_forward_act': (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_void_p, c_int,
                                          c_void_p, c_int, c_void_p]),
    'cae_t_corr_s1': (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_int, c_int, c_void_p, c_void_p, c_int, c_void_p,
                               c_int, c_void_p]),
    'cae_t_wgrad_s1': (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p]),
    'cae_t_act_backward': (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    'cae_t_im2col_s2': (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    'cae_t_col2im_s2': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    'cae_t_pointwise': (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int,
                                 c_void_p]),
    'cae_t_wgrad_pointwise': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    'cae_t_gdn_saved_elems': (c_size_t, [ctypes.c_long, c_int]),
    'cae_t_gdn_forward_save': (c_int, [c_void_p, ctypes.c_long, c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p]),
    'cae_t_gdn_backward_fused': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_int,
                                          c_void_p, c_void_p, c_void_p, c_void_p]),
    'cae_t_fold_to_bf16': (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    'cae_t_col2im_s1r': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    'cae_t_im2col_s1r': (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    'cae_t_pointwise_acc': (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_int, c_void_p]),
    'cae_t_fold_acc': (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    'cae_t_pyramid_down': (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    'cae_t_msssim_level_fwd': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, ctypes.POINTER(ctypes.c_double), c_int, ctypes.c_double,
                                       ctypes.c_double, c_void_p, c_void_p, c_size_t, c_void_p]),
    'cae_t_msssim_level_bwd': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, ctypes.POINTER(ctypes.c_double), c_int, ctypes.c_double,
                                       ctypes.c_double, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    'cae_t_avgpool2_bwd': (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p]),
    'cae_t_bn_moments': (c_int, [c_void_p, c_void_p, c_int, c_int, ctypes.c_long, c_void_p, c_void_p, c_void_p]),
    'cae_t_bn_affine': (c_int, [c_void_p, c_void_p, c_int, c_int, ctypes.c_long, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    'cae_t_colsum': (c_int, [c_void_p, ctypes.c_long, c_int, c_void_p, c_void_p]),
    'cae_t_density_params': (c_int, [c_int, c_int]),
    'cae_t_reparam_forward': (c_int, [c_void_p, ctypes.c_long, ctypes.c_float, ctypes.c_float, c_void_p, c_void_p]),
    'cae_t_reparam_backward': (c_int, [c_void_p, c_void_p, ctypes.c_long, ctypes.c_float, c_void_p, c_void_p]),
    'cae_t_density_forward': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, ctypes.c_float, c_void_p,
                                      c_void_p, c_void_p]),
    'cae_t_density_backward': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, ctypes.c_float,
                                       c_void_p, c_void_p, c_void_p]),
    'cae_t_clip_adam': (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p,
                                c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    'cae_t_sample_patches': (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                     c_void_p, c_void_p, ctypes.c_uint64, ctypes.c_uint32, c_float, c_int, c_int, c_int,
                                     c_void_p, c_void_p]),
    'cae_t_sample_labeled_patches': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p,
                                             c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, ctypes.c_uint64,
                                             ctypes.c_uint32, c_float, c_int, c_int, c_int, c_int, c_void_p, c_size_t,
                                             c_void_p, c_void_p, c_void_p]),
    'cae_t_elastic_deform': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_size_t, c_void_p,
                                     c_void_p, c_void_p]),
    'cae_t_elastic_deform_workspace': (c_size_t, [c_int, c_int, c_int]),
    'cae_cpu_budget': (c_int, []),
    'cae_coder_lockstep': (c_int, []),
    'cae_coder_threads': (c_int, [c_int, c_int]),
    'cae_pmf_to_quantized_cdf': (c_int, [c_void_p, c_int, c_int, c_void_p]),
    'cae_rans_encode_batch': (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_int]),
    'cae_rans_encode_packed': (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_int]),
    'cae_rans_decode_batch': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_int]),
    'cae_rans_encode_workspace': (c_int, [c_void_p, c_int, c_int, ctypes.POINTER(c_size_t)]),
    'cae_rans_encode_device': (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_size_t, c_void_p, c_void_p, c_void_p,
                                       c_size_t, c_void_p]),
    'cae_rans_decode_device': (c_int, [c_void_p, c_void_p, c_size_t, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    'cae_door_create': (c_int, [c_void_p, c_void_p, c_int, c_int, ctypes.POINTER(c_void_p)]),
    'cae_door_destroy': (None, [c_void_p]),
    'cae_door_encode': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, ctypes.POINTER(c_void_p),
                                ctypes.POINTER(c_size_t)]),
    'cae_door_decode_shape': (c_int, [c_void_p, c_void_p, c_size_t, ctypes.POINTER(c_int), ctypes.POINTER(c_int),
                                      ctypes.POINTER(c_int)]),
    'cae_door_decode': (c_int, [c_void_p, c_void_p, c_size_t, c_void_p, c_size_t]),
    'cae_door_stats': (c_int, [c_void_p, c_void_p, c_int, c_int]),
    'cae_door_hold': (c_int, [c_void_p, c_int]),
    'cae_seg_plan': (c_int, [c_void_p, c_void_p, c_int]),
    'cae_seg_workspace_bytes': (c_int, [c_void_p, c_int, c_int, c_int, c_void_p]),
    'cae_seg_weight_count': (c_int, [c_void_p]),
    'cae_seg_create': (c_int, [c_void_p, c_void_p, c_int, ctypes.POINTER(c_void_p)]),
    'cae_seg_destroy': (None, [c_void_p]),
    'cae_seg_stage_count': (c_int, [c_void_p]),
    'cae_seg_forward': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    'cae_seg_last_ticket': (ctypes.c_int64, []),
    'cae_seg_range_check': (c_int, [c_void_p, ctypes.c_int64]),
    'cae_seg_packed_halves': (c_size_t, [c_int, c_int, c_int, c_int, c_int]),
    'cae_seg_pack': (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_size_t]),
    'cae_seg_tile': (None, [ctypes.POINTER(c_int), ctypes.POINTER(c_int)]),
    'cae_seg_predict': (c_int, [c_void_p, c_void_p, c_int, c_int, c_size_t, c_float, c_int, c_void_p, c_void_p, c_void_p,
                                c_void_p, c_size_t, c_void_p]),
    'cae_seg_predict_workspace': (c_size_t, [c_int, c_int, c_size_t]),
    'cae_seg_roc_hist': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p,
                                 c_size_t, c_void_p]),
    'cae_seg_roc_workspace': (c_size_t, [c_int, c_int, c_int, c_int]),
    'cae_seg_roc_blocks': (c_int, [c_int, c_int, c_int, c_int]),
    'cae_seg_score_hist': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p,
                                   c_void_p, c_size_t, c_void_p]),
    'cae_seg_score_workspace': (c_size_t, [c_int, c_int, c_int, c_int, c_int]),
    'cae_seg_components': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_size_t,
                                   c_void_p]),
    'cae_seg_components_workspace': (c_size_t, [c_int, c_int, c_int]),
    'cae_seg_object_cover': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_size_t, c_void_p]),
    'cae_seg_object_cover_workspace': (c_size_t, [c_int, c_int, c_int]),
    'cae_seg_object_counts': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_size_t, c_float, c_int, c_void_p,
                                      c_void_p, c_size_t, c_void_p]),
    'cae_seg_object_counts_workspace': (c_size_t, [c_int, c_int, c_size_t]),
    'cae_seg_object_roc_hist': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int,
                                        c_void_p, c_void_p, c_size_t, c_void_p]),
    'cae_seg_object_roc_workspace': (c_size_t, [c_int, c_int, c_int, c_int]),
    'cae_seg_object_distances': (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_size_t, c_void_p]),
    'cae_seg_object_distances_workspace': (c_size_t, [c_int, c_int, c_int]),
    'cae_seg_weight_map': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_float, c_float, c_int, c_size_t,
                                   c_void_p, c_void_p, c_void_p]),
    'cae_mask_gray': (c_int, [c_void_p, c_int, c_size_t, c_void_p, c_void_p, c_void_p]),
    'cae_mask_hist': (c_int, [c_void_p, c_void_p, c_int, c_size_t, c_void_p, c_void_p, c_size_t, c_void_p]),
    'cae_mask_hist_workspace': (c_size_t, [c_int, c_size_t]),
    'cae_mask_hist_fold': (c_size_t, []),
    'cae_mask_threshold': (c_int, [c_void_p, c_void_p, c_int, c_size_t, c_void_p, c_void_p]),
    'cae_mask_label': (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_size_t, c_void_p]),
    'cae_mask_label_workspace': (c_size_t, [c_int, c_int, c_int]),
    'cae_mask_area_filter': (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_size_t,
                                     c_void_p]),
    'cae_mask_area_workspace': (c_size_t, [c_int, c_int, c_int]),
    'cae_mask_within': (c_int, [c_void_p, c_int, c_size_t, c_int, c_void_p, c_void_p]),
    'cae_mask_downscale': (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_size_t, c_size_t, c_int, c_void_p, c_void_p]),
    'cae_tile_byte_hist': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_size_t, c_void_p]),
    'cae_tile_byte_hist_workspace': (c_size_t, [c_int, c_int, c_int, c_int]),
    'cae_tile_byte_hist_blocks': (c_int, [c_int, c_int, c_int, c_int]),
    'cae_persistent_launch': (c_int, [c_int] * 5 + [ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(c_int)]),
    'cae_seg_set_weights': (c_int, [c_void_p, c_void_p, c_int, c_void_p]),
    'cae_seg_pack_dev': (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_size_t, c_void_p, c_void_p]),
    'cae_seg_conv2d_workspace': (c_size_t, [c_int] * 6),
    'cae_seg_conv2d': (c_int, [c_void_p] * 4 + [c_int] * 6 + [c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    'cae_seg_wgrad_splits': (c_int, [c_int] * 6),
    'cae_seg_wgrad_workspace': (c_size_t, [c_int] * 6),
    'cae_seg_wgrad': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int,
                              c_int, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    'cae_seg_norm_workspace': (c_size_t, [c_int, c_int]),
    'cae_seg_norm_relu_backward': (c_int, [c_void_p] * 4 + [c_int, c_int, c_size_t] + [c_void_p] * 4 + [c_size_t, c_void_p]),
    'cae_seg_channel_sums_workspace': (c_size_t, [c_int, c_int]),
    'cae_seg_channel_sums': (c_int, [c_void_p, c_int, c_int, c_size_t, c_void_p, c_void_p, c_size_t, c_void_p]),
}

CAE_ANALYSIS, CAE_SYNTHESIS = 0, 1
FMT_U8_HWC, FMT_F32_NCHW = 0, 1


class CaeError(RuntimeError):
    pass


def build(verbose: bool = False) -> str:
    """Compile libcae_hip.so for gfx950 with hipcc (cross-compiles without a GPU)."""
    cmd = ['make', '-j8', '-C', os.path.join(_HERE, 'csrc'), 'all']
    if not verbose:
        cmd.insert(1, '-s')
    subprocess.check_call(cmd)
    return LIB_PATH


def lib() -> ctypes.CDLL:
    global _lib
    with _lock:
        if _lib is None:
            if not os.path.exists(LIB_PATH):
                raise ImportError(
                    f'{LIB_PATH} not found: the HIP extension is not built and there is no CPU fallback. '
                    'Run `make -C cnn_autoencoder_amd/csrc` (needs hipcc).')
            L = ctypes.CDLL(LIB_PATH)
            for name, (res, args) in SYMBOLS.items():
                fn = getattr(L, name)  # AttributeError if the library does not export it
                fn.restype = res
                fn.argtypes = args
            _lib = L
    return _lib


def check(rc: int):
    if rc != 0:
        msg = lib().cae_last_error().decode('utf-8', 'replace')
        if rc == -1:
            raise ValueError(msg)  # the reference / compressai raise ValueError on bad shapes
        if rc == -6:
            raise FloatingPointError(msg)  # the call left the valid range of its kernels
        raise CaeError(f'libcae_hip error {rc}: {msg}')


def require_gpu() -> torch.device:
    if not torch.cuda.is_available():
        raise RuntimeError('cnn_autoencoder_amd: no HIP device is visible; the MI355X hot path has no CPU fallback')
    return torch.device('cuda', torch.cuda.current_device())


def stream_ptr() -> int:
    return torch.cuda.current_stream().cuda_stream


class Handle:
    """Owns one cae_model_t."""

    def __init__(self, c_org: int, c_net: int, c_bn: int, level: int, ks: int):
        self._h = c_void_p()
        check(lib().cae_model_create(c_org, c_net, c_bn, level, ks, ctypes.byref(self._h)))

    @property
    def ptr(self):
        return self._h

    def close(self):
        if self._h:
            lib().cae_model_destroy(self._h)
            self._h = c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
