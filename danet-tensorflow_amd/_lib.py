'''
ctypes binding of the twenty-one HIP libraries (the C ABIs declared in include/danet*_hip.h): the core
libdanet_hip.so and the conv, dropout, prep, mix, speed, reverb, metric, noise, level, wavloss, gclip, dpcl, neval,
stitch, bss, stoi, phase, online, causal and tonline extension libraries.  Each is described
once, by a record of ALL_LIBRARIES, LATER_LIBRARIES, EXTENSIONS or MORE_EXTENSIONS; one loader (_load) and one error check (_check) serve them all.

There is NO fallback: if a shared library is missing or a call fails, a
RuntimeError is raised.  PyTorch is used only to own device memory and streams;
tensors cross the boundary as raw device pointers.
'''
import collections
import ctypes
import os
import threading

import torch

_CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'csrc')

c_int, c_i64, c_f32, c_sz, c_p, c_u32 = (ctypes.c_int, ctypes.c_int64, ctypes.c_float,
                                         ctypes.c_size_t, ctypes.c_void_p, ctypes.c_uint32)
c_f64 = ctypes.c_double


class GemmPack(ctypes.Structure):
    '''danet_gemm_pack_t (include/danet_hip.h)'''
    _fields_ = [('src', c_p), ('stride_n', ctypes.c_longlong), ('stride_k', ctypes.c_longlong),
                ('N', c_int), ('K', c_int), ('out', c_p), ('out_bytes', c_sz)]


class GemmProblem(ctypes.Structure):
    '''danet_gemm_problem_t (include/danet_hip.h)'''
    _fields_ = [('A', c_p), ('lda', c_int), ('B', c_p), ('ldb', c_int), ('C', c_p), ('ldc', c_int),
                ('M', c_int), ('N', c_int), ('bias', c_p), ('beta', c_f32)]


# name -> (restype, argtypes); mirrors include/danet_hip.h
PROTOTYPES = {
    'danet_abi_version': (c_int, []),
    'danet_last_error': (ctypes.c_char_p, []),
    'danet_set_option': (c_int, [ctypes.c_char_p, c_int]),
    'danet_get_option': (c_int, [ctypes.c_char_p, ctypes.POINTER(c_int)]),
    'danet_reset_options': (None, []),
    'danet_option_count': (c_int, []),
    'danet_option_name': (ctypes.c_char_p, [c_int]),
    'danet_workspace_bytes': (c_sz, [c_int, ctypes.POINTER(c_i64), c_int]),
    'danet_stft_num_frames': (c_int, [c_i64, c_int, c_int]),
    'danet_stft': (c_int, [c_p, c_int, c_i64, c_int, c_int, c_p, c_p, c_p]),
    'danet_istft': (c_int, [c_p, c_int, c_int, c_int, c_int, c_p, c_p, c_p, c_p, c_sz]),
    'danet_frontend_fwd': (c_int, [c_p, c_int, c_int, c_i64, c_p, c_p, c_p, c_p, c_p, c_p, c_p]),
    'danet_reattach_phase': (c_int, [c_p, c_int, c_int, c_i64, c_p, c_p, c_p, c_p]),
    'danet_center': (c_int, [c_p, c_int, c_int, c_int, c_p, c_int, c_int, c_p, c_int, c_int, c_p]),
    'danet_gemm_f32': (c_int, [c_p, c_int, c_int, c_int, c_int, c_int, c_p, c_int, c_p, c_int,
                               c_p, c_int, c_p, c_f32, c_p, c_sz, c_int]),
    'danet_gemm_f32_streamk': (c_int, [c_p, c_int, c_int, c_int, c_int, c_int, c_p, c_int, c_p, c_int,
                                       c_p, c_int, c_p, c_f32, c_p, c_sz]),
    'danet_gemm_f32_streamk_grouped': (c_int, [c_p, c_int, c_int, c_int, c_int,
                                               ctypes.POINTER(GemmProblem), c_int, c_p, c_sz]),
    'danet_gemm_f32_streamk_kcat': (c_int, [c_p, c_int, c_int, c_int, c_int,
                                            c_int, c_p, c_int, c_p, c_int, c_int, c_p, c_int, c_p, c_int,
                                            c_p, c_int, c_p, c_f32, c_p, c_sz]),
    'danet_gemm_pack_weights': (c_int, [c_p, c_int, ctypes.POINTER(GemmPack)]),
    'danet_gemm_x6': (c_int, [c_p, c_int, c_int, c_int, c_p, c_int, c_p, c_int, c_p, c_int, c_p,
                              c_p, c_int, c_p, c_p, c_sz]),
    'danet_gemm_x6_tn_grouped': (c_int, [c_p, c_int, c_int, ctypes.POINTER(GemmProblem), c_p, c_sz]),
    'danet_colsum_f32': (c_int, [c_p, c_int, c_int, c_p, c_int, c_p, c_f32, c_p, c_sz]),
    'danet_lstm_fwd': (c_int, [c_p, c_int, c_int, c_int, c_int, c_p, c_p, c_p, c_p, c_int,
                               c_p, c_int, c_p, c_p, c_p, c_p, c_p, c_sz, c_p, c_int]),
    'danet_lstm_fwd_prefill': (c_int, [c_p, c_int, c_int, c_int, c_int, ctypes.POINTER(c_p),
                                       ctypes.POINTER(c_p)]),
    'danet_encoder_prologue': (c_int, [c_p, c_int, c_int, c_int, c_p, c_int, c_int, c_p, c_int, c_int, c_p,
                                       c_int, c_int, c_int, c_int, ctypes.POINTER(c_p), ctypes.POINTER(c_p),
                                       ctypes.POINTER(c_p)]),
    'danet_lstm_train_prefill': (c_int, [c_p, c_int, c_int, c_int, c_int, c_int, c_int, ctypes.POINTER(c_p),
                                         ctypes.POINTER(c_p), ctypes.POINTER(c_p)]),
    'danet_lstm_fwd_fused_supported': (c_int, [c_int, c_int, c_int, c_int, c_int]),
    'danet_lstm_fwd_fused': (c_int, [c_p, c_int, c_int, c_int, c_int, c_p, c_int, c_int, c_p, c_p,
                                     c_int, c_p, c_p, c_p, c_int, c_p, c_p, c_p, c_p, c_p, c_sz, c_p,
                                     c_int]),
    'danet_lstm_bwd': (c_int, [c_p, c_int, c_int, c_int, c_int, c_p, c_int, c_p, c_p, c_int,
                               c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_f32, c_p, c_sz, c_p, c_int]),
    'danet_lstm_bwd_db_supported': (c_int, [c_int, c_int, c_int, c_int]),
    'danet_lstm_bwd_db_reduce': (c_int, [c_p, c_int, c_int, c_int, c_int, c_p, c_p, c_f32, c_p, c_sz]),
    'danet_next_launch_events': (c_int, [c_p, c_p]),
    'danet_event_create': (c_int, [ctypes.POINTER(c_p)]),
    'danet_event_destroy': (c_int, [c_p]),
    'danet_stream_wait_event': (c_int, [c_p, c_p]),
    'danet_attractor_truth_fwd': (c_int, [c_p, c_int, c_int, c_int, c_i64, c_int, c_p, c_p, c_p,
                                          c_f32, c_p, c_p, c_p, c_sz]),
    'danet_attractor_truth_bwd': (c_int, [c_p, c_int, c_int, c_int, c_i64, c_int, c_p, c_p, c_p,
                                          c_p, c_f32, c_p]),
    'danet_attractor_truth_bwd_sep': (c_int, [c_p, c_int, c_int, c_int, c_i64, c_int, c_p, c_p, c_p, c_p,
                                              c_f32, c_p, c_p, c_int, c_int, c_p, c_p, c_p, c_p, c_f32,
                                              c_p, c_p, c_p]),
    'danet_attractor_anchor_fwd': (c_int, [c_p, c_int, c_int, c_i64, c_int, c_int, c_p, c_p, c_p,
                                           c_p, c_p, c_p, c_p, c_sz]),
    'danet_separate_fwd': (c_int, [c_p, c_int, c_int, c_int, c_i64, c_int, c_p, c_p, c_p, c_p, c_p]),
    'danet_separate_bwd': (c_int, [c_p, c_int, c_int, c_int, c_i64, c_int, c_p, c_p, c_p, c_p,
                                   c_p, c_p, c_p, c_sz]),
    'danet_separate_pit_bwd': (c_int, [c_p, c_int, c_int, c_int, c_int, c_i64, c_int, c_p, c_p, c_p,
                                       c_p, c_p, c_p, c_p, c_f32, c_p, c_p, c_p, c_p, c_sz]),
    'danet_separate_pit_fwd_records': (c_int, [c_p, c_int, c_int, c_int, c_int, c_i64, c_int, c_p, c_p,
                                               c_p, c_p, c_p, c_p, c_p, c_p]),
    'danet_separate_pit_final': (c_int, [c_p, c_int, c_int, c_i64, c_f32, c_p, c_p, c_p, c_p]),
    'danet_attractor_anchor_bwd_embed': (c_int, [c_p, c_int, c_int, c_i64, c_int, c_int, c_p, c_p, c_p,
                                                 c_p, c_p, c_p, c_p, c_p, c_sz]),
    'danet_attractor_anchor_bwd_embed_sep': (c_int, [c_p, c_int, c_int, c_i64, c_int, c_int, c_p, c_p, c_p,
                                                     c_p, c_p, c_p, c_int, c_int, c_p, c_p, c_p, c_p, c_p,
                                                     c_f32, c_p, c_p, c_p, c_sz, c_p]),
    'danet_attractor_anchor_bwd_anchors': (c_int, [c_p, c_int, c_int, c_i64, c_int, c_int, c_p, c_p,
                                                   c_p, c_sz, c_f32]),
    'danet_pit_mse_fwd': (c_int, [c_p, c_int, c_int, c_int, c_i64, c_p, c_p, c_p, c_f32, c_p,
                                  c_p, c_p, c_p, c_sz]),
    'danet_pit_mse_bwd': (c_int, [c_p, c_int, c_int, c_int, c_i64, c_p, c_p, c_p, c_p, c_f32, c_p, c_p]),
    'danet_leaky_relu': (c_int, [c_p, c_i64, c_p, c_p, c_f32, c_p]),
    'danet_adam_clip_step': (c_int, [c_p, c_i64, c_p, c_p, c_p, c_p, c_f32, c_f32, c_f32, c_f32,
                                     c_f32, c_f32, c_int]),
}

class ConvDesc(ctypes.Structure):
    '''danet_conv_desc_t (include/danet_conv_hip.h)'''
    _fields_ = [('B', c_int), ('Cin', c_int), ('Cout', c_int), ('T', c_int), ('F', c_int), ('k', c_int),
                ('pool', c_int), ('d2s', c_int), ('alpha', c_f32),
                ('x_stride', c_i64 * 4), ('y_stride', c_i64 * 4)]


_CD = ctypes.POINTER(ConvDesc)
# name -> (restype, argtypes); mirrors include/danet_conv_hip.h
CONV_PROTOTYPES = {
    'danet_conv_abi_version': (c_int, []),
    'danet_conv_last_error': (ctypes.c_char_p, []),
    'danet_conv_workspace_bytes': (c_sz, [c_int, _CD]),
    'danet_conv_fwd': (c_int, [c_p, _CD, c_p, c_p, c_p, c_p, c_p]),
    'danet_conv_bwd_data': (c_int, [c_p, _CD, c_p, c_p, c_p, c_p, c_p]),
    'danet_conv_bwd_weight': (c_int, [c_p, _CD, c_p, c_p, c_p, c_p, c_p, c_p, c_int, c_p, c_sz]),
    'danet_conv_add': (c_int, [c_p, c_i64, c_p, c_p, c_p]),
}
CONV_WS_BWD_WEIGHT = 0

# name -> (restype, argtypes); mirrors include/danet_dropout_hip.h
DROPOUT_PROTOTYPES = {
    'danet_dropout_abi_version': (c_int, []),
    'danet_dropout_last_error': (ctypes.c_char_p, []),
    'danet_dropout_apply': (c_int, [c_p, c_i64, c_i64, c_p, c_i64, c_p, c_i64, c_u32, c_f32, c_u32, c_u32,
                                    c_u32, c_u32]),
}

# name -> (restype, argtypes); mirrors include/danet_prep_hip.h
PREP_PROTOTYPES = {
    'danet_prep_abi_version': (c_int, []),
    'danet_prep_last_error': (ctypes.c_char_p, []),
    'danet_prep_num_frames': (c_int, [c_i64, c_int, c_int]),
    'danet_prep_workspace_bytes': (c_sz, [c_int]),
    'danet_prep_stft_plan': (c_int, [c_p, c_int, c_p, c_p, c_sz]),
    'danet_prep_stft_batch': (c_int, [c_p, c_int, c_p, c_i64, c_p, c_int, c_int, c_int, c_int, c_int, c_p, c_p,
                                      c_p, c_i64]),
}

# name -> (restype, argtypes); mirrors include/danet_mix_hip.h
MIX_PROTOTYPES = {
    'danet_mix_abi_version': (c_int, []),
    'danet_mix_last_error': (ctypes.c_char_p, []),
    'danet_mix_workspace_bytes': (c_sz, [c_int, c_i64]),
    'danet_mix_power': (c_int, [c_p, c_int, c_p, c_i64, c_p, c_p, c_i64, c_p, c_p, c_sz]),
    'danet_mix_scale_c64': (c_int, [c_p, c_int, c_int, c_int, c_p, c_i64, c_p]),
}

# name -> (restype, argtypes); mirrors include/danet_speed_hip.h
SPEED_PROTOTYPES = {
    'danet_speed_abi_version': (c_int, []),
    'danet_speed_last_error': (ctypes.c_char_p, []),
    'danet_speed_out_len': (c_i64, [c_i64, c_int]),
    'danet_speed_resample': (c_int, [c_p, c_int, c_p, c_i64, c_p, c_p, c_p, c_i64]),
}

# name -> (restype, argtypes); mirrors include/danet_reverb_hip.h
REVERB_PROTOTYPES = {
    'danet_reverb_abi_version': (c_int, []),
    'danet_reverb_last_error': (ctypes.c_char_p, []),
    'danet_reverb_apply': (c_int, [c_p, c_int, c_p, c_i64, c_p, c_p, c_int, c_p, c_i64]),
}

# name -> (restype, argtypes); mirrors include/danet_metric_hip.h
METRIC_PROTOTYPES = {
    'danet_metric_abi_version': (c_int, []),
    'danet_metric_last_error': (ctypes.c_char_p, []),
    'danet_metric_workspace_bytes': (c_sz, [c_int, c_int, c_int, c_int, c_int]),
    'danet_metric_synth': (c_int, [c_p, c_int, c_int, c_int, c_int, c_int, c_p, c_p, c_p, c_p]),
    'danet_metric_gram': (c_int, [c_p, c_int, c_int, c_i64, c_p, c_p]),
    'danet_metric_si_sdr': (c_int, [c_p, c_int, c_int, c_p, c_p, c_p, c_p]),
}

# name -> (restype, argtypes); mirrors include/danet_noise_hip.h
NOISE_PROTOTYPES = {
    'danet_noise_abi_version': (c_int, []),
    'danet_noise_last_error': (ctypes.c_char_p, []),
    'danet_noise_frontend_fwd': (c_int, [c_p, c_int, c_int, c_i64, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p]),
}

# name -> (restype, argtypes); mirrors include/danet_level_hip.h
LEVEL_PROTOTYPES = {
    'danet_level_abi_version': (c_int, []),
    'danet_level_last_error': (ctypes.c_char_p, []),
    'danet_level_workspace_bytes': (c_sz, [c_int, c_i64]),
    'danet_level_activity': (c_int, [c_p, c_int, c_p, c_i64, c_p, c_p, c_i64, c_f64, c_i64, c_p, c_p, c_p, c_sz]),
}

# name -> (restype, argtypes); mirrors include/danet_wavloss_hip.h
WAVLOSS_PROTOTYPES = {
    'danet_wavloss_abi_version': (c_int, []),
    'danet_wavloss_last_error': (ctypes.c_char_p, []),
    'danet_wavloss_fwd': (c_int, [c_p, c_int, c_int, c_p, c_p, c_p, c_p, c_p, c_p, c_p]),
    'danet_wavloss_bwd': (c_int, [c_p, c_int, c_int, c_int, c_int, c_int, c_p, c_p, c_p, c_p, c_p, c_p, c_p]),
}

# name -> (restype, argtypes); mirrors include/danet_gclip_hip.h
GCLIP_PROTOTYPES = {
    'danet_gclip_abi_version': (c_int, []),
    'danet_gclip_last_error': (ctypes.c_char_p, []),
    'danet_gclip_partials': (c_int, [c_i64]),
    'danet_gclip_sumsq': (c_int, [c_p, c_i64, c_p, c_p, c_int]),
    'danet_gclip_adam_step': (c_int, [c_p, c_i64, c_p, c_p, c_p, c_p, c_f32, c_f32, c_f32, c_f32, c_f32, c_f32, c_int,
                                      c_f64, c_p, c_int, c_p]),
}

# name -> (restype, argtypes); mirrors include/danet_dpcl_hip.h
DPCL_PROTOTYPES = {
    'danet_dpcl_abi_version': (c_int, []),
    'danet_dpcl_last_error': (ctypes.c_char_p, []),
    'danet_dpcl_chunks': (c_int, [c_i64]),
    'danet_dpcl_workspace_bytes': (c_sz, [c_int, c_i64, c_int, c_int]),
    'danet_dpcl_stats': (c_int, [c_p, c_int, c_i64, c_int, c_int, c_p, c_p, c_p, c_sz]),
    'danet_dpcl_finalize': (c_int, [c_p, c_int, c_i64, c_int, c_int, c_p, c_sz, c_p, c_f32, c_p, c_p, c_p, c_p, c_p]),
    'danet_dpcl_bwd': (c_int, [c_p, c_int, c_i64, c_int, c_int, c_p, c_p, c_p, c_p, c_p, c_f32, c_p]),
}

# name -> (restype, argtypes); mirrors include/danet_neval_hip.h
NEVAL_PROTOTYPES = {
    'danet_neval_abi_version': (c_int, []),
    'danet_neval_last_error': (ctypes.c_char_p, []),
    'danet_neval_workspace_bytes': (c_sz, [c_int, c_int, c_int, c_int, c_int]),
    'danet_neval_synth': (c_int, [c_p, c_int, c_int, c_int, c_int, c_int, c_p, c_p, c_p, c_p, c_p, c_p]),
    'danet_neval_gram': (c_int, [c_p, c_int, c_int, c_i64, c_p, c_p]),
    'danet_neval_si_sdr': (c_int, [c_p, c_int, c_int, c_p, c_p, c_p, c_p]),
}

# name -> (restype, argtypes); mirrors include/danet_stitch_hip.h
STITCH_PROTOTYPES = {
    'danet_stitch_abi_version': (c_int, []),
    'danet_stitch_last_error': (ctypes.c_char_p, []),
    'danet_stitch_chunks': (c_int, [c_int, c_int, c_int]),
    'danet_stitch_workspace_bytes': (c_sz, [c_int, c_int, c_int, c_int, c_int]),
    'danet_stitch_affinity': (c_int, [c_p, c_int, c_int, c_int, c_int, c_int, c_p, c_p, c_sz]),
    'danet_stitch_assign': (c_int, [c_p, c_int, c_int, c_int, c_int, c_int, c_p, c_sz, c_p, c_p]),
    'danet_stitch_merge': (c_int, [c_p, c_int, c_int, c_int, c_int, c_int, c_p, c_p, c_p, c_p, c_p]),
}

# name -> (restype, argtypes); mirrors include/danet_bss_hip.h
BSS_PROTOTYPES = {
    'danet_bss_abi_version': (c_int, []),
    'danet_bss_last_error': (ctypes.c_char_p, []),
    'danet_bss_workspace_bytes': (c_sz, [c_int, c_int, c_int]),
    'danet_bss_xcorr': (c_int, [c_p, c_int, c_int, c_i64, c_int, c_p, c_p, c_p, c_p]),
    'danet_bss_systems': (c_int, [c_p, c_int, c_int, c_int, c_p, c_p, c_p, c_p, c_p, c_p]),
    'danet_bss_chol_solve': (c_int, [c_p, c_int, c_int, c_int, c_p, c_p, c_p]),
    'danet_bss_finalize': (c_int, [c_p, c_int, c_int, c_int, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_int, c_int,
                                   c_p, c_p, c_p, c_p]),
}

# name -> (restype, argtypes); mirrors include/danet_stoi_hip.h
STOI_PROTOTYPES = {
    'danet_stoi_abi_version': (c_int, []),
    'danet_stoi_last_error': (ctypes.c_char_p, []),
    'danet_stoi_workspace_bytes': (c_sz, [c_int, c_int, c_i64, c_int, c_int]),
    'danet_stoi_resample': (c_int, [c_p, c_int, c_int, c_i64, c_int, c_int, c_p, c_p, c_p]),
    'danet_stoi_frames': (c_int, [c_p, c_int, c_int, c_i64, c_p, c_p, c_p, c_p, c_p, c_p, c_p]),
    'danet_stoi_bands': (c_int, [c_p, c_int, c_int, c_i64, c_p, c_p, c_p, c_p, c_p, c_p, c_p]),
    'danet_stoi_segments': (c_int, [c_p, c_int, c_int, c_int, c_p, c_p, c_p]),
    'danet_stoi_finalize': (c_int, [c_p, c_int, c_int, c_int, c_p, c_p, c_p, c_int, c_int, c_p, c_p, c_p, c_p, c_p]),
}

# name -> (restype, argtypes); mirrors include/danet_phase_hip.h
PHASE_PROTOTYPES = {
    'danet_phase_abi_version': (c_int, []),
    'danet_phase_last_error': (ctypes.c_char_p, []),
    'danet_phase_workspace_bytes': (c_sz, [c_int, c_int, c_int, c_int, c_int]),
    'danet_phase_init': (c_int, [c_p, c_int, c_int, c_int, c_int, c_int, c_int, c_p, c_p, c_p, c_p, c_p]),
    'danet_phase_synth': (c_int, [c_p, c_int, c_int, c_int, c_int, c_int, c_p, c_p, c_p]),
    'danet_phase_project': (c_int, [c_p, c_int, c_int, c_int, c_int, c_int, c_p, c_p, c_p, c_p]),
}

# name -> (restype, argtypes); mirrors include/danet_online_hip.h
ONLINE_PROTOTYPES = {
    'danet_online_abi_version': (c_int, []),
    'danet_online_last_error': (ctypes.c_char_p, []),
    'danet_online_state_bytes': (c_sz, [c_int, c_int]),
    'danet_online_init': (c_int, [c_p, c_int, c_int, c_int, c_p, c_p]),
    'danet_online_scan': (c_int, [c_p, c_int, c_int, c_int, c_int, c_int, c_int, c_f64, c_int, c_i64, c_f64, c_p, c_p,
                                  c_p, c_p]),
    'danet_online_separate': (c_int, [c_p, c_int, c_int, c_int, c_int, c_int, c_int, c_p, c_p, c_p, c_p]),
}

# name -> (restype, argtypes); mirrors include/danet_causal_hip.h
CAUSAL_PROTOTYPES = {
    'danet_causal_abi_version': (c_int, []),
    'danet_causal_last_error': (ctypes.c_char_p, []),
    'danet_causal_center_fwd': (c_int, [c_p, c_int, c_int, c_int, c_p, c_int, c_int, c_p, c_int, c_int, c_p]),
    'danet_causal_center_bwd': (c_int, [c_p, c_int, c_int, c_int, c_p, c_int, c_int, c_p, c_int, c_int]),
    'danet_causal_lstm_ws_bytes': (c_sz, [c_int, c_int, c_int, c_int]),
    'danet_causal_lstm_block': (c_int, [c_p, c_int, c_int, c_int, c_int, c_int, c_p, c_int, ctypes.POINTER(c_p),
                                        ctypes.POINTER(c_p), c_p, c_p, c_p, c_int, c_p, c_sz]),
    'danet_causal_project': (c_int, [c_p, c_int, c_int, c_int, c_p, c_int, c_p, c_int, c_p, c_int]),
}

# name -> (restype, argtypes); mirrors include/danet_tonline_hip.h
TONLINE_PROTOTYPES = {
    'danet_tonline_abi_version': (c_int, []),
    'danet_tonline_last_error': (ctypes.c_char_p, []),
    'danet_tonline_frame_sums': (c_int, [c_p, c_int, c_int, c_int, c_int, c_int, c_p, c_p, c_p, c_p, c_p]),
    'danet_tonline_scan': (c_int, [c_p, c_int, c_int, c_int, c_int, c_f64, c_int, c_f64, c_p, c_p, c_p, c_p]),
    'danet_tonline_scan_bwd': (c_int, [c_p, c_int, c_int, c_int, c_int, c_f64, c_int, c_p, c_p, c_p]),
    'danet_tonline_sums_bwd': (c_int, [c_p, c_int, c_int, c_int, c_int, c_int, c_p, c_p, c_p, c_p]),
    'danet_tonline_separate_bwd': (c_int, [c_p, c_int, c_int, c_int, c_int, c_int, c_int, c_p, c_p, c_p, c_p, c_p,
                                           c_p]),
}

# ---- the libraries -------------------------------------------------------------
# Twenty-one shared objects, each with a header, an ABI version and a prototype table of its own (the core's
# table stays exactly the core header's).  A missing library is a hard error for every one of them.
# To add one: a record here, its prototype table above, a source directory csrc/<name>/ with an
# exports.map (and a record in _build.py), and a header include/danet_<name>_hip.h.  LIBRARIES stays the five
# records the per-record tests are written against, by position, ALL_LIBRARIES those and SPEED, and
# _build.LIBRARIES the same six, LATER_LIBRARIES the seventh, EXTENSIONS the next seven; every library after them is
# APPENDED to MORE_EXTENSIONS, here and in _build.py (which builds them in build_all), and is served by the same
# Library record type, _load and _check.
#   name: '' for the core; so: the file under csrc/; path_var / handle_var: the module globals that hold
#   its path (read when it is loaded: tests and tools assign to it) and its CDLL (None until then);
#   prefix: danet_<p>abi_version and danet_<p>last_error follow from it; needs: who needs it, for the
#   message of a missing file
Library = collections.namedtuple('Library', 'name so path_var handle_var prototypes abi prefix needs')
CONV_ABI_VERSION = DROPOUT_ABI_VERSION = PREP_ABI_VERSION = MIX_ABI_VERSION = SPEED_ABI_VERSION = 1
REVERB_ABI_VERSION = 1

CORE = Library('', 'libdanet_hip.so', 'LIB_PATH', '_lib', PROTOTYPES, 7, 'danet_',
               'the HIP extension is required')
CONV = Library('conv', 'libdanet_conv_hip.so', 'CONV_LIB_PATH', '_conv', CONV_PROTOTYPES, CONV_ABI_VERSION,
               'danet_conv_', 'the conv-bilstm-v1 encoder needs the HIP extension library')
# loaded at the first call with keep < 1 only: a run with DROPOUT_KEEP_PROB = 1 never maps it
DROPOUT = Library('dropout', 'libdanet_dropout_hip.so', 'DROPOUT_LIB_PATH', '_dropout', DROPOUT_PROTOTYPES,
                  DROPOUT_ABI_VERSION, 'danet_dropout_', 'DROPOUT_KEEP_PROB < 1 needs the HIP extension library')
# loaded at the first use of the `wavdir` dataset (ops.stft_batch) only: a run with any other DATASET_TYPE
# never maps it
PREP = Library('prep', 'libdanet_prep_hip.so', 'PREP_LIB_PATH', '_prep', PREP_PROTOTYPES, PREP_ABI_VERSION,
               'danet_prep_', 'the wavdir dataset needs the HIP extension library')
# loaded at the first wavdir batch with MIX_SNR_RANGE or MIX_LEVEL_RANGE set only (ops.mix_power /
# ops.mix_scale_): a run with both keys null never maps it
MIX = Library('mix', 'libdanet_mix_hip.so', 'MIX_LIB_PATH', '_mix', MIX_PROTOTYPES, MIX_ABI_VERSION,
              'danet_mix_', 'MIX_SNR_RANGE / MIX_LEVEL_RANGE need the HIP extension library')
# loaded at the first wavdir TRAIN batch with SPEED_PERTURB_RANGE set only (ops.speed_resample): a run with
# the key null, and every evaluation sweep, never maps it
SPEED = Library('speed', 'libdanet_speed_hip.so', 'SPEED_LIB_PATH', '_speed', SPEED_PROTOTYPES, SPEED_ABI_VERSION,
                'danet_speed_', 'SPEED_PERTURB_RANGE needs the HIP extension library')
# loaded at the first wavdir TRAIN batch with REVERB_RT60_MAX set only (ops.reverb_apply): a run with the key
# null, and every evaluation sweep, never maps it
REVERB = Library('reverb', 'libdanet_reverb_hip.so', 'REVERB_LIB_PATH', '_reverb', REVERB_PROTOTYPES,
                 REVERB_ABI_VERSION, 'danet_reverb_', 'REVERB_RT60_MAX needs the HIP extension library')
LIBRARIES = (CORE, CONV, DROPOUT, PREP, MIX)
ALL_LIBRARIES = LIBRARIES + (SPEED,)
LATER_LIBRARIES = (REVERB,)
# The three tuples above are closed (tests pin them by length and content).  EXTENSIONS was the open tuple of the
# eighth to the fourteenth library (MORE_EXTENSIONS, below it, is today's).
# loaded at the first valid / test step with EVAL_SI_SDR true only (ops.si_sdr): a run with the key null never
# maps it
METRIC_ABI_VERSION = 1
METRIC = Library('metric', 'libdanet_metric_hip.so', 'METRIC_LIB_PATH', '_metric', METRIC_PROTOTYPES,
                 METRIC_ABI_VERSION, 'danet_metric_', 'EVAL_SI_SDR needs the HIP extension library')
# loaded at the first wavdir TRAIN step with NOISE_DIR set only (ops.noise_frontend): a run with the key null, and
# every evaluation sweep, never maps it
NOISE_ABI_VERSION = 1
NOISE = Library('noise', 'libdanet_noise_hip.so', 'NOISE_LIB_PATH', '_noise', NOISE_PROTOTYPES,
                NOISE_ABI_VERSION, 'danet_noise_', 'NOISE_DIR needs the HIP extension library')
# loaded when the first power table of a wavdir dataset with MIX_LEVEL_MEASURE = "active" is measured only
# (ops.level_activity): a run with the key null never maps it
LEVEL_ABI_VERSION = 1
LEVEL = Library('level', 'libdanet_level_hip.so', 'LEVEL_LIB_PATH', '_level', LEVEL_PROTOTYPES,
                LEVEL_ABI_VERSION, 'danet_level_', 'MIX_LEVEL_MEASURE needs the HIP extension library')
# loaded at the first train step (or forward pass with the train branch) of a model built with TRAIN_LOSS = "si-sdr"
# only (ops.si_sdr_loss): a run with the key null or "pit-mse" never maps it
WAVLOSS_ABI_VERSION = 1
WAVLOSS = Library('wavloss', 'libdanet_wavloss_hip.so', 'WAVLOSS_LIB_PATH', '_wavloss', WAVLOSS_PROTOTYPES,
                  WAVLOSS_ABI_VERSION, 'danet_wavloss_', 'TRAIN_LOSS = "si-sdr" needs the HIP extension library')
# loaded at the first train step of a model built with GRAD_CLIP_NORM set only (ops.grad_sumsq): a run with the key
# null never maps it
GCLIP_ABI_VERSION = 1
GCLIP = Library('gclip', 'libdanet_gclip_hip.so', 'GCLIP_LIB_PATH', '_gclip', GCLIP_PROTOTYPES,
                GCLIP_ABI_VERSION, 'danet_gclip_', 'GRAD_CLIP_NORM needs the HIP extension library')
# loaded at the first train step (or forward pass with the train branch) of a model built with DPCL_WEIGHT set only
# (ops.dpcl_loss): a run with the key null never maps it
DPCL_ABI_VERSION = 1
DPCL = Library('dpcl', 'libdanet_dpcl_hip.so', 'DPCL_LIB_PATH', '_dpcl', DPCL_PROTOTYPES,
               DPCL_ABI_VERSION, 'danet_dpcl_', 'DPCL_WEIGHT needs the HIP extension library')
# loaded at the first valid / test step that is handed a noise component with EVAL_SI_SDR true only
# (ops.si_sdr_noisy): a run with NOISE_EVAL_DIR or EVAL_SI_SDR null never maps it
NEVAL_ABI_VERSION = 1
NEVAL = Library('neval', 'libdanet_neval_hip.so', 'NEVAL_LIB_PATH', '_neval', NEVAL_PROTOTYPES,
                NEVAL_ABI_VERSION, 'danet_neval_', 'NOISE_EVAL_DIR with EVAL_SI_SDR needs the HIP extension library')
# loaded at the first Model.infer of a recording longer than INFER_CHUNK_LEN frames only (ops.stitch): a run with the
# key null, and an input of at most one chunk, never maps it
STITCH_ABI_VERSION = 1
STITCH = Library('stitch', 'libdanet_stitch_hip.so', 'STITCH_LIB_PATH', '_stitch', STITCH_PROTOTYPES,
                 STITCH_ABI_VERSION, 'danet_stitch_', 'INFER_CHUNK_LEN needs the HIP extension library')
EXTENSIONS = (METRIC, NOISE, LEVEL, WAVLOSS, GCLIP, DPCL, NEVAL)
# EXTENSIONS is closed too by now: tests/test_neval_cpu.py pins it as the six libraries in front of NEVAL and NEVAL, here
# and in _build.py.  MORE_EXTENSIONS is the tuple every library from the fifteenth on is appended to, here and in
# _build.py (build_all runs over it after EXTENSIONS); a test of a new library asserts `ITS_RECORD in MORE_EXTENSIONS`
# and that its record follows the ones that were there, never the tuple's length or what else it holds.
# loaded at the first valid / test step with EVAL_BSS_SDR true only (ops.bss_eval): a run with the key null never
# maps it
BSS_ABI_VERSION = 1
BSS = Library('bss', 'libdanet_bss_hip.so', 'BSS_LIB_PATH', '_bss', BSS_PROTOTYPES,
              BSS_ABI_VERSION, 'danet_bss_', 'EVAL_BSS_SDR needs the HIP extension library')
# loaded at the first valid / test step with EVAL_STOI true only (ops.stoi_eval): a run with the key null never maps it
STOI_ABI_VERSION = 1
STOI = Library('stoi', 'libdanet_stoi_hip.so', 'STOI_LIB_PATH', '_stoi', STOI_PROTOTYPES,
               STOI_ABI_VERSION, 'danet_stoi_', 'EVAL_STOI needs the HIP extension library')
# loaded at the first infer / valid step of a model built with PHASE_REFINE_ITERS set only (ops.phase_refine): a run
# with the key null never maps it
PHASE_ABI_VERSION = 1
PHASE = Library('phase', 'libdanet_phase_hip.so', 'PHASE_LIB_PATH', '_phase', PHASE_PROTOTYPES,
                PHASE_ABI_VERSION, 'danet_phase_', 'PHASE_REFINE_ITERS needs the HIP extension library')
# loaded at the first infer / valid step of a model whose inference estimator is "online", on a recording longer than
# the hold, only (ops.online_attractors / ops.online_separate): a run with any other estimator never maps it
ONLINE_ABI_VERSION = 1
ONLINE = Library('online', 'libdanet_online_hip.so', 'ONLINE_LIB_PATH', '_online', ONLINE_PROTOTYPES,
                 ONLINE_ABI_VERSION, 'danet_online_', 'the "online" estimator needs the HIP extension library')
# loaded at the first forward pass of the `lstm-causal` encoder or the first Model.open_stream only (ops.causal_*): a
# run with another encoder and INFER_STREAM_BLOCK null never maps it
CAUSAL_ABI_VERSION = 1
CAUSAL = Library('causal', 'libdanet_causal_hip.so', 'CAUSAL_LIB_PATH', '_causal', CAUSAL_PROTOTYPES,
                 CAUSAL_ABI_VERSION, 'danet_causal_', 'the lstm-causal encoder and streaming inference need the HIP '
                 'extension library')
# loaded at the first train step (or forward pass with the train branch) of a model built with TRAIN_ESTIMATOR_METHOD =
# "truth-online" only (ops.TruthOnlineAttractorFn / ops.OnlineSeparateFn): a run with another train estimator, and
# every valid_step, infer and stream session, never maps it
TONLINE_ABI_VERSION = 1
TONLINE = Library('tonline', 'libdanet_tonline_hip.so', 'TONLINE_LIB_PATH', '_tonline', TONLINE_PROTOTYPES,
                  TONLINE_ABI_VERSION, 'danet_tonline_', 'TRAIN_ESTIMATOR_METHOD = "truth-online" needs the HIP '
                  'extension library')
MORE_EXTENSIONS = (STITCH, BSS, STOI, PHASE, ONLINE, CAUSAL, TONLINE)

# DANET_LIB_PATH: an A/B build of the same sources (_build.build_variant), never a different backend
LIB_PATH = os.environ.get('DANET_LIB_PATH') or os.path.join(_CSRC, CORE.so)
CONV_LIB_PATH = os.path.join(_CSRC, CONV.so)
DROPOUT_LIB_PATH = os.path.join(_CSRC, DROPOUT.so)
PREP_LIB_PATH = os.path.join(_CSRC, PREP.so)
MIX_LIB_PATH = os.path.join(_CSRC, MIX.so)
SPEED_LIB_PATH = os.path.join(_CSRC, SPEED.so)
REVERB_LIB_PATH = os.path.join(_CSRC, REVERB.so)
METRIC_LIB_PATH = os.path.join(_CSRC, METRIC.so)
NOISE_LIB_PATH = os.path.join(_CSRC, NOISE.so)
LEVEL_LIB_PATH = os.path.join(_CSRC, LEVEL.so)
WAVLOSS_LIB_PATH = os.path.join(_CSRC, WAVLOSS.so)
GCLIP_LIB_PATH = os.path.join(_CSRC, GCLIP.so)
DPCL_LIB_PATH = os.path.join(_CSRC, DPCL.so)
NEVAL_LIB_PATH = os.path.join(_CSRC, NEVAL.so)
STITCH_LIB_PATH = os.path.join(_CSRC, STITCH.so)
BSS_LIB_PATH = os.path.join(_CSRC, BSS.so)
STOI_LIB_PATH = os.path.join(_CSRC, STOI.so)
PHASE_LIB_PATH = os.path.join(_CSRC, PHASE.so)
ONLINE_LIB_PATH = os.path.join(_CSRC, ONLINE.so)
CAUSAL_LIB_PATH = os.path.join(_CSRC, CAUSAL.so)
TONLINE_LIB_PATH = os.path.join(_CSRC, TONLINE.so)
_lib = _conv = _dropout = _prep = _mix = _speed = _reverb = _metric = _noise = _level = _wavloss = _gclip = _dpcl = None
_neval = _stitch = _bss = _stoi = _phase = _online = _causal = _tonline = None
_lock = threading.Lock()


class DanetHipError(RuntimeError):
    pass


def _load(spec, loaded=None):
    '''dlopen the library of `spec` (after torch, so both share ONE libamdhip64), bind its prototype
    table, check its ABI version and store the handle in its module global; then call `loaded`'''
    g = globals()
    if g[spec.handle_var] is None:
        with _lock:
            if g[spec.handle_var] is None:
                path = g[spec.path_var]
                if not os.path.exists(path):
                    raise DanetHipError(
                        '%s not found at %s -- %s (there is no CPU fallback); build it with '
                        '`python -c "import __graft_entry__ as g; g.build()"`' % (spec.so, path, spec.needs))
                # torch already mapped its bundled libamdhip64.so (SONAME libamdhip64.so.7);
                # our DT_NEEDED of the same SONAME resolves to that copy.
                lib = ctypes.CDLL(path, mode=ctypes.RTLD_LOCAL)
                for name, (res, args) in spec.prototypes.items():
                    fn = getattr(lib, name)      # AttributeError if the symbol is missing
                    fn.restype = res
                    fn.argtypes = args
                if getattr(lib, spec.prefix + 'abi_version')() != spec.abi:
                    raise DanetHipError('%s ABI version mismatch' % spec.so)
                g[spec.handle_var] = lib
                if loaded is not None:
                    loaded()
    return g[spec.handle_var]


def _check(spec, rc):
    '''raise the error behind the return code `rc` != 0 of a call into the library of `spec`'''
    msg = getattr(_load(spec), spec.prefix + 'last_error')()
    raise DanetHipError('%s error %d: %s' % (spec.so[:-3], rc, msg.decode() if msg else '?'))


def bytes_or_raise(nbytes, check):
    '''the result of a library's *_workspace_bytes, or its error raised through that library's `check`:
    (size_t)-1 says the arguments were refused and last_error says why'''
    if nbytes == ctypes.c_size_t(-1).value:
        check(-1)
    return nbytes


# Every load_*() answers from its global once that is set: load() runs at every kernel launch.
def load():
    if _lib is not None:
        return _lib
    return _load(CORE, apply_env_options)


def load_conv():
    if _conv is not None:
        return _conv
    return _load(CONV)


def conv_check(rc):
    if rc != 0:
        _check(CONV, rc)


def conv_ws_bytes(op, desc):
    '''danet_conv_workspace_bytes(op, desc)'''
    return bytes_or_raise(load_conv().danet_conv_workspace_bytes(op, ctypes.byref(desc)), conv_check)


def load_dropout():
    if _dropout is not None:
        return _dropout
    return _load(DROPOUT)


def dropout_check(rc):
    if rc != 0:
        _check(DROPOUT, rc)


def load_prep():
    if _prep is not None:
        return _prep
    return _load(PREP)


def prep_check(rc):
    if rc != 0:
        _check(PREP, rc)


def load_mix():
    if _mix is not None:
        return _mix
    return _load(MIX)


def mix_check(rc):
    if rc != 0:
        _check(MIX, rc)


def load_speed():
    if _speed is not None:
        return _speed
    return _load(SPEED)


def speed_check(rc):
    if rc != 0:
        _check(SPEED, rc)


def load_reverb():
    if _reverb is not None:
        return _reverb
    return _load(REVERB)


def reverb_check(rc):
    if rc != 0:
        _check(REVERB, rc)


def load_metric():
    if _metric is not None:
        return _metric
    return _load(METRIC)


def metric_check(rc):
    if rc != 0:
        _check(METRIC, rc)


def load_noise():
    if _noise is not None:
        return _noise
    return _load(NOISE)


def noise_check(rc):
    if rc != 0:
        _check(NOISE, rc)


def load_level():
    if _level is not None:
        return _level
    return _load(LEVEL)


def level_check(rc):
    if rc != 0:
        _check(LEVEL, rc)


def load_wavloss():
    if _wavloss is not None:
        return _wavloss
    return _load(WAVLOSS)


def wavloss_check(rc):
    if rc != 0:
        _check(WAVLOSS, rc)


def load_gclip():
    if _gclip is not None:
        return _gclip
    return _load(GCLIP)


def gclip_check(rc):
    if rc != 0:
        _check(GCLIP, rc)


def load_dpcl():
    if _dpcl is not None:
        return _dpcl
    return _load(DPCL)


def dpcl_check(rc):
    if rc != 0:
        _check(DPCL, rc)


def load_neval():
    if _neval is not None:
        return _neval
    return _load(NEVAL)


def neval_check(rc):
    if rc != 0:
        _check(NEVAL, rc)


def load_stitch():
    if _stitch is not None:
        return _stitch
    return _load(STITCH)


def stitch_check(rc):
    if rc != 0:
        _check(STITCH, rc)


def load_bss():
    if _bss is not None:
        return _bss
    return _load(BSS)


def bss_check(rc):
    if rc != 0:
        _check(BSS, rc)


def load_stoi():
    if _stoi is not None:
        return _stoi
    return _load(STOI)


def stoi_check(rc):
    if rc != 0:
        _check(STOI, rc)


def load_phase():
    if _phase is not None:
        return _phase
    return _load(PHASE)


def phase_check(rc):
    if rc != 0:
        _check(PHASE, rc)


def load_online():
    if _online is not None:
        return _online
    return _load(ONLINE)


def online_check(rc):
    if rc != 0:
        _check(ONLINE, rc)


def load_causal():
    if _causal is not None:
        return _causal
    return _load(CAUSAL)


def causal_check(rc):
    if rc != 0:
        _check(CAUSAL, rc)


def load_tonline():
    if _tonline is not None:
        return _tonline
    return _load(TONLINE)


def tonline_check(rc):
    if rc != 0:
        _check(TONLINE, rc)


# ---- switches ------------------------------------------------------------------
# USER switches (README): DANET_GEMM_X6, DANET_LSTM_FWD_FUSED, DANET_SIDE_STREAMS, DANET_FEED_MODE,
# DANET_OVERLAP_ALLREDUCE, DANET_ALLREDUCE_TAIL_RATIO, DANET_MAX_STEPS_IN_FLIGHT, DANET_STATUS_HOST, DANET_FUSE_HEADS,
# DANET_LSTM_SPIN_LIMIT, DANET_LSTM_FAULT_INJECT, DANET_LIB_PATH (+ three of bench.py).  Everything
# else -- the schedule knobs of the exact-fp32 fallback kernels, placement and fork details, the
# remaining library options -- is an EXPERT setting behind ONE variable:
#     DANET_EXPERT="streamk=5,grouped_dw=0,gemm_yield=8"
# (names: the lower-case module constants of ops.py / model.py that call `expert()`, and the library
# options of csrc/options.h).  Defaults are the shipped, measured configuration.
_expert = None
_expert_seen = set()      # every name some module has asked for (typos in DANET_EXPERT are reported, below)


def expert(name, default):
    '''value of the expert setting `name` (DANET_EXPERT="name=value,...") or `default`, as
    type(default)'''
    global _expert
    if _expert is None:
        _expert = {}
        for item in os.environ.get('DANET_EXPERT', '').split(','):
            if item.strip():
                k, _, v = item.partition('=')
                _expert[k.strip().lower()] = v.strip()
    _expert_seen.add(name.lower())
    v = _expert.get(name.lower())
    if v is None:
        return default
    if isinstance(default, bool):
        return v not in ('0', 'false', 'no', '')
    return type(default)(v)


USER_OPTIONS = ('lstm_fwd_fused', 'lstm_spin_limit', 'lstm_fault_inject')   # library options with a DANET_<NAME> variable


# ---- library options ---------------------------------------------------------
# The C library never reads the environment (include/danet_hip.h); the DANET_* overrides of
# its options live HERE: option `lstm_fwd_fused` <- env DANET_LSTM_FWD_FUSED, applied when the
# library is loaded (and by apply_env_options(), which tests call to restore the defaults).
def option_names():
    lib = _lib
    return [lib.danet_option_name(i).decode() for i in range(lib.danet_option_count())]


def apply_env_options():
    '''reset every option to its default, then apply DANET_<NAME> from the environment'''
    lib = _lib
    lib.danet_reset_options()
    for name in option_names():
        v = os.environ.get('DANET_' + name.upper()) if name in USER_OPTIONS else None
        if v is None or v.strip() == '':
            v = expert(name, '')
        if v != '':
            check(lib.danet_set_option(name.encode(), int(v)))
    # a key of DANET_EXPERT that neither a module constant nor a library option answers to is a typo: say so
    # (the library is loaded at the first kernel call, after ops.py / model.py have read their settings)
    unknown = sorted(set(_expert or {}) - _expert_seen)
    if unknown:
        import warnings
        warnings.warn('DANET_EXPERT: unknown setting(s) %s (known: the lower-case constants of ops.py / model.py '
                      'that call _lib.expert(), and the library options %s)' % (unknown, option_names()))


def set_option(name, value):
    check(load().danet_set_option(name.encode(), int(value)))


def get_option(name):
    v = c_int(0)
    check(load().danet_get_option(name.encode(), ctypes.byref(v)))
    return v.value


def check(rc):
    if rc != 0:
        _check(CORE, rc)


# DANET_WS_* (include/danet_hip.h)
(WS_ISTFT, WS_GEMM, WS_GEMM_STREAMK, WS_COLSUM, WS_LSTM, WS_ATTRACTOR_TRUTH, WS_ATTRACTOR_ANCHOR,
 WS_SEPARATE_BWD, WS_SEPARATE_PIT, WS_SEPARATE_PIT_RECORDS, WS_PIT_MSE, WS_CENTER_MEAN,
 WS_GEMM_X6, WS_GEMM_PACK, WS_GEMM_X6_TN, WS_SEPARATE_PIT_GRAD) = range(16)


def ws_bytes(op, *dims):
    '''danet_workspace_bytes(op, dims): scratch bytes of the entry point behind DANET_WS_<op>'''
    arr = (c_i64 * len(dims))(*[int(d) for d in dims])
    return bytes_or_raise(load().danet_workspace_bytes(op, arr, len(dims)), check)


def ptr(t):
    '''raw device pointer of a torch tensor (None -> NULL)'''
    if t is None:
        return None
    return t.data_ptr()


def stream():
    return torch.cuda.current_stream().cuda_stream


# ---- scratch ---------------------------------------------------------------
_ws = {}


def workspace(nbytes, device, tag=None):
    '''per-(device, stream, tag) grow-only scratch, zero-initialised; safe because
    every library call is stream-ordered on the current stream and finishes with
    `ws` before the next call on that stream starts.'''
    key = (device.index if device.index is not None else torch.cuda.current_device(),
           torch.cuda.current_stream().cuda_stream, tag)
    t = _ws.get(key)
    if t is None or t.numel() < nbytes:
        t = torch.zeros(max(int(nbytes), 1 << 20), dtype=torch.uint8, device=device)
        _ws[key] = t
    return t


# ---- optional per-kernel timing (HIP events on the launch stream) ------------
_prof = None
_prof_only = None
_prof_on = True


def profile_start(only=None):
    '''only: optional set of labels to time (every event pair costs ~1 us of stream
    time, so a timed benchmark region instruments just the kernel it reports)'''
    global _prof, _prof_only
    if torch.cuda.is_available():
        prepare_timing(64)          # (a no-op after prepare_timing())
    _prof = {}
    _prof_only = set(only) if only else None


def profile_enable(flag):
    '''pause / resume event recording inside a profile_start()..profile_stop() window'''
    global _prof_on
    _prof_on = bool(flag)


def profile_stop():
    '''-> {label: (n_launches, total_ms)}; synchronises'''
    global _prof
    p, _prof = _prof, None
    torch.cuda.synchronize()
    out = {}
    for label, evs in (p or {}).items():
        out[label] = (len(evs), sum(a.elapsed_time(b) for a, b in evs))
    return out


# labels whose ONE kernel launch carries the event pair on its own dispatch packet
# (danet_next_launch_events) instead of two event records around the call: the recurrent kernels.
# A record in front of the launch delays it by a few microseconds, enough for the side stream's
# weight-gradient group to get its workgroups onto the CUs first -- the persistent kernel then
# starts piecemeal and the bracket reads 50 us more than the kernel takes in an untimed step.
ATTACHED_LABELS = frozenset(('lstm_fwd', 'lstm_bwd'))
_aux_stream = None
_event_pool = []


def _timing_event():
    '''a timing-enabled event whose native handle exists (torch creates it on first record; that
    record goes to a stream nobody else uses).  profile_start() fills a pool, so that a timed
    region creates neither a stream nor events (a stream created inside a 20-step region cost it
    5-6 ms on some boxes).'''
    global _aux_stream
    if _event_pool:
        return _event_pool.pop()
    return _timing_event_new()


def prepare_timing(n=384):
    '''create the side stream and a pool of timing events NOW (call before the warm-up steps of a
    benchmark: creating them, and the synchronisation behind it, must not sit at the start of a
    timed region)'''
    made = False
    while len(_event_pool) < n:
        _event_pool.append(_timing_event_new())
        made = True
    if made:
        torch.cuda.synchronize()


def _timing_event_new():
    global _aux_stream
    if _aux_stream is None:
        _aux_stream = torch.cuda.Stream()
    e = torch.cuda.Event(enable_timing=True)
    e.record(_aux_stream)
    return e


class timed(object):
    '''with timed('label'): <one library call>  -- records a start/end event pair
    on the current stream (the stream the kernels are launched on) when
    profiling is enabled; free otherwise.  Labels in ATTACHED_LABELS: the pair rides on the
    call's own kernel launch.'''
    __slots__ = ('label', 'tag', 'a', 'b')

    def __init__(self, label, tag=None):
        self.label, self.tag = label, tag

    def __enter__(self):
        self.a = self.b = None
        if _prof is not None and _prof_on and (_prof_only is None or self.label in _prof_only):
            if self.label in ATTACHED_LABELS:
                self.a, self.b = _timing_event(), _timing_event()
                check(load().danet_next_launch_events(self.a.cuda_event, self.b.cuda_event))
            else:
                self.a = torch.cuda.Event(enable_timing=True)
                self.a.record()
        return self

    def __exit__(self, *exc):
        if self.a is not None and _prof is not None:
            b = self.b
            if b is None:
                b = torch.cuda.Event(enable_timing=True)
                b.record()
            _prof.setdefault(self.label, []).append((self.a, b))
            if self.tag:      # per-call-site breakdown next to the per-entry-point total
                _prof.setdefault(self.label + ':' + self.tag, []).append((self.a, b))
        return False
