"""ctypes binding of libkfnet_hip.so (include/kfnet_hip.h).

The product path has NO CPU fallback: if the library is missing, or an entry point
returns an error, a KfnError is raised.
"""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, 'libkfnet_hip.so')

KFN_OK = 0
ABI_VERSION = 13
COMM_ID_BYTES = 128
EPI_NONE, EPI_L2NORM, EPI_EXP_CH3, EPI_EXP_1E2 = 0, 1, 2, 3
OPERAND_F32, OPERAND_F16, OPERAND_F16X3 = 0, 1, 2
ACT_F32, ACT_F16 = 0, 1
LAYOUT_NHWC, LAYOUT_C16 = 0, 1                            # kfn_conv_desc.x_layout / y_layout (KFN_LAYOUT_*)
PNG_OK, PNG_UNSUPPORTED, PNG_ERROR = 0, 1, 2
WINO_ORDER_AUTO, WINO_ORDER_M_FAST, WINO_ORDER_N_FAST = 0, 1, 2
CFG_128x256 = 9
CFG_256x64, CFG_256x256, CFG_256x256_W8 = 12, 13, 14
WINO_FORM_F43_FOUR_WAVE, WINO_FORM_F43_EIGHT_WAVE = 2, 3   # kfn_conv_desc.wino_form for kfn_conv2d_winograd_f43
WINO_FORM_S2_EIGHT_WAVE = 4                                # ... for kfn_conv2d_winograd_s2
WINO_FORM_S2_F42 = 5                                       # ... its polyphase + F(4,2) form (wino_s2c_kernel)
PNP_OK, PNP_TOO_FEW_POINTS, PNP_NO_HYPOTHESIS = 0, 1, 2      # kfn_pnp_ransac info[:, 0] (KFN_PNP_*)
PNP_MAX_HYPOTHESES = 1024
PNP_SAMPLE_CONFIDENCE, PNP_SAMPLE_CONFIDENCE_SQ = 1, 2       # kfn_pnp_sample_desc.mode (KFN_PNP_SAMPLE_*)
PNP_MAX_CONFIDENCE_CAP = 4096.
POSE_UPDATED, POSE_MISSING, POSE_REJECTED, POSE_INIT, POSE_NONE = 0, 1, 2, 3, 4     # kfn_pose_filter flags (KFN_POSE_*)
POSE_MODEL_WALK, POSE_MODEL_VELOCITY = 0, 1                                        # kfn_pose_track_desc.model (KFN_POSE_MODEL_*)
PACK_FORWARD, PACK_INPUT_GRAD_S1, PACK_INPUT_GRAD_S2 = 0, 1, 2     # kfn_pack_conv_weights kind (KFN_PACK_*)
CFG_AUTO, CFG_160x128, CFG_128x128, CFG_128x64, CFG_128x32, CFG_64x64, CFG_256x32, CFG_192x64 = 0, 1, 2, 3, 4, 5, 6, 7


class KfnError(RuntimeError):
    pass


class SizedStructure(C.Structure):
    """A descriptor whose first field is `struct_size`: filled in here with the size of the concrete structure unless the
    caller set it.  The library copies that many bytes and reads every later field as 0, so such a struct can grow at its
    end without breaking older hosts."""

    def __init__(self, *args, **kw):
        super(SizedStructure, self).__init__(*args, **kw)
        if not self.struct_size:
            self.struct_size = C.sizeof(type(self))


class ConvDesc(SizedStructure):
    """kfn_conv_desc (include/kfnet_hip.h); tests/test_host_logic.py::test_conv_desc_matches_header_and_integration_doc
    keeps its field list equal to the header's and INTEGRATION.md's."""
    _fields_ = [(n, C.c_int32) for n in (
        'struct_size', 'N', 'H', 'W', 'Cin', 'ldx', 'Cout', 'cout_pad', 'ldy', 'kh', 'kw', 'stride',
        'transposed', 'relu', 'epilogue', 'config', 'operand_dtype', 'wino_order', 'wino_form',
        'x_dtype', 'y_dtype', 'k_step', 'weights_path', 'x_layout', 'y_layout')]


class WinoPlan(SizedStructure):
    """kfn_wino_plan (include/kfnet_hip.h): what a Winograd entry point launches for a descriptor.  `kernel` is a
    KFN_WINO_KERNEL_* value, WINO_KERNEL_NAMES[kernel] the name the ops report for it (the fp32 / 16-byte-store instantiations
    without their template argument)."""
    _fields_ = [(n, C.c_int32) for n in (
        'struct_size', 'kernel', 'threads', 'lds_bytes', 'workgroups', 'tiles_m', 'tiles_n', 'tiles_per_block',
        'channels_per_group', 'n_group', 'wide_store', 'k_split', 'ss_per_split')]


(WINO_KERNEL_WINO2_WIDE, WINO_KERNEL_WINO2_DWORD, WINO_KERNEL_WINO3, WINO_KERNEL_WINO3_F16, WINO_KERNEL_WINO3_PAIR, WINO_KERNEL_WINO4,
 WINO_KERNEL_WINO4B, WINO_KERNEL_S2, WINO_KERNEL_S2_F16, WINO_KERNEL_S2B, WINO_KERNEL_S2C, WINO_KERNEL_S2C_PERSISTENT) = range(1, 13)
WINO_KERNEL_NAMES = (None, 'wino2_kernel', 'wino2_kernel', 'wino3_kernel', 'wino3_kernel<true>', 'wino3_pair_kernel',
                     'wino4_kernel', 'wino4b_kernel', 'wino_s2_kernel', 'wino_s2_kernel<true>', 'wino_s2b_kernel',
                     'wino_s2c_kernel', 'wino_s2c_pkernel')


def winograd_launch_plan(desc, k_split=0, cu_count=0, y_low_bits=0):
    """kfn_winograd_launch_plan: the WinoPlan of the launch the Winograd entry points make for `desc` (k_split 0: the plain
    one, >= 1: the split-K one), or None when they refuse it (kfn_last_error says why)."""
    plan = WinoPlan()
    if load().kfn_winograd_launch_plan(C.byref(desc), k_split, cu_count, y_low_bits, C.byref(plan)) != KFN_OK:
        return None
    return plan


class KalmanDesc(C.Structure):
    _fields_ = [('S', C.c_int32), ('T', C.c_int32), ('H', C.c_int32), ('W', C.c_int32),
                ('t0', C.c_int32), ('reset_period', C.c_int32),
                ('min_uncertainty', C.c_double), ('nis_gate', C.c_float),
                ('has_transform', C.c_int32), ('transform', C.c_float * 12)]


class PnPDesc(SizedStructure):
    """kfn_pnp_desc (include/kfnet_hip.h, ABI 11); `struct_size` is filled in here, as for ConvDesc."""
    _fields_ = [('struct_size', C.c_int32), ('B', C.c_int32), ('h', C.c_int32), ('w', C.c_int32), ('ld', C.c_int32),
                ('t0', C.c_int32), ('seed', C.c_uint32), ('hypotheses', C.c_int32), ('refine_iters', C.c_int32),
                ('min_points', C.c_int32), ('fx', C.c_float), ('fy', C.c_float), ('u', C.c_float), ('v', C.c_float),
                ('cell_stride', C.c_int32), ('min_confidence', C.c_float), ('inlier_px', C.c_float)]


class PnPUncDesc(SizedStructure):
    """kfn_pnp_unc_desc (include/kfnet_hip.h); `struct_size` is filled in here."""
    _fields_ = [('struct_size', C.c_int32), ('weighted', C.c_int32), ('pixel_sigma', C.c_float)]


class PnPSampleDesc(SizedStructure):
    """kfn_pnp_sample_desc (include/kfnet_hip.h); `struct_size` is filled in here."""
    _fields_ = [('struct_size', C.c_int32), ('mode', C.c_int32), ('confidence_cap', C.c_float)]


class KabschDesc(SizedStructure):
    """kfn_kabsch_desc (include/kfnet_hip.h); `struct_size` is filled in here."""
    _fields_ = [('struct_size', C.c_int32), ('B', C.c_int32), ('h', C.c_int32), ('w', C.c_int32), ('ld', C.c_int32),
                ('ldp', C.c_int32), ('t0', C.c_int32), ('seed', C.c_uint32), ('hypotheses', C.c_int32),
                ('refine_iters', C.c_int32), ('min_points', C.c_int32), ('min_confidence', C.c_float), ('inlier_m', C.c_float),
                ('weighted', C.c_int32), ('point_sigma', C.c_float)]


class PoseFilterDesc(SizedStructure):
    """kfn_pose_filter_desc (include/kfnet_hip.h); `struct_size` is filled in here."""
    _fields_ = [('struct_size', C.c_int32), ('S', C.c_int32), ('T', C.c_int32), ('rot_sigma', C.c_float),
                ('trans_sigma', C.c_float), ('gate', C.c_float), ('max_rejects', C.c_int32)]


class PoseTrackDesc(SizedStructure):
    """kfn_pose_track_desc (include/kfnet_hip.h); `struct_size` is filled in here."""
    _fields_ = [('struct_size', C.c_int32), ('S', C.c_int32), ('T', C.c_int32), ('model', C.c_int32), ('smooth', C.c_int32),
                ('rot_sigma', C.c_float), ('trans_sigma', C.c_float), ('rot_rate_sigma', C.c_float),
                ('trans_rate_sigma', C.c_float), ('gate', C.c_float), ('max_rejects', C.c_int32)]


class CoordLossDesc(SizedStructure):
    """kfn_coord_loss_desc (include/kfnet_hip.h); `struct_size` is filled in here."""
    _fields_ = [('struct_size', C.c_int32), ('B', C.c_int32), ('h', C.c_int32), ('w', C.c_int32), ('ld_pred', C.c_int32),
                ('ld_dpred', C.c_int32), ('label_stride', C.c_int32), ('img_stride', C.c_int32),
                ('has_transform', C.c_int32), ('transform', C.c_float * 12), ('has_loss_clip', C.c_int32),
                ('loss_clip', C.c_float), ('smooth_weight', C.c_float), ('dist_threshold', C.c_double),
                ('min_uncertainty', C.c_double)]


class AugmentDesc(SizedStructure):
    """kfn_augment_desc (include/kfnet_hip.h); `struct_size` is filled in here.  kfnet_amd.augment.descriptor derives it."""
    _fields_ = ([(n, C.c_int32) for n in ('struct_size', 'B', 'H', 'W', 'label_stride', 'mode', 'has_rotation', 'has_colour')] +
                [('rot', C.c_float * 6)] + [(n, C.c_float) for n in ('y0', 'dy', 'x0', 'dx')] +
                [(n, C.c_int32) for n in ('new_h', 'new_w', 'off_y', 'off_x')] +
                [(n, C.c_float) for n in ('scale_y', 'scale_x', 'delta', 'factor')])


class DepthLabelsDesc(SizedStructure):
    """kfn_depth_labels_desc (include/kfnet_hip.h); `struct_size` is filled in here.  kfnet_amd.labels.DepthCamera.descriptor
    derives it."""
    _fields_ = ([(n, C.c_int32) for n in ('struct_size', 'B', 'H', 'W', 'stride', 'ld_out', 'registration', 'raw_min', 'raw_max')] +
                [(n, C.c_float) for n in ('u', 'v', 'inv_fx', 'inv_fy', 'kx', 'ky', 'ud', 'vd', 'scale')])


class LabelMomentsDesc(SizedStructure):
    """kfn_label_moments_desc (include/kfnet_hip.h); `struct_size` is filled in here."""
    _fields_ = ([(n, C.c_int32) for n in ('struct_size', 'B', 'h', 'w', 'ld', 'reserved')] + [('pivot', C.c_double * 3)])


class RenderDesc(SizedStructure):
    """kfn_render_desc (include/kfnet_hip.h); `struct_size` is filled in here.  kfnet_amd.render.render_descriptor derives it."""
    _fields_ = ([(n, C.c_int32) for n in ('struct_size', 'B', 'V', 'N', 'H', 'W', 'stride', 'ld_labels', 'raw_min', 'raw_max')] +
                [(n, C.c_float) for n in ('u', 'v', 'inv_fx', 'inv_fy', 'fx', 'fy', 'near', 'scale')])


class FuseDesc(SizedStructure):
    """kfn_fuse_desc (include/kfnet_hip.h); `struct_size` is filled in here.  kfnet_amd.fuse.fuse_descriptor derives it."""
    _fields_ = ([(n, C.c_int32) for n in ('struct_size', 'nx', 'ny', 'nz', 'B', 'H', 'W', 'raw_min', 'raw_max')] +
                [(n, C.c_float) for n in ('ox', 'oy', 'oz', 'voxel', 'trunc', 'near', 'scale', 'max_weight', 'min_weight',
                                          'dfx', 'dfy', 'du', 'dv', 'fx', 'fy', 'u', 'v')])


class TrackDesc(SizedStructure):
    """kfn_track_desc (include/kfnet_hip.h); `struct_size` is filled in here.  kfnet_amd.track.track_descriptor derives it."""
    _fields_ = ([(n, C.c_int32) for n in ('struct_size', 'nx', 'ny', 'nz', 'H', 'W', 'levels', 'level', 'raw_min', 'raw_max',
                                          'min_pairs', 'traj_rows', 'slot')] +
                [(n, C.c_float) for n in ('ox', 'oy', 'oz', 'voxel', 'trunc', 'near', 'far', 'scale', 'min_weight', 'dfx', 'dfy', 'du',
                                          'dv', 'pyr_dist', 'jump', 'dist_max', 'cos_min', 'pivot_floor', 'min_share', 'max_rms',
                                          'max_step_m', 'max_step_rad')])


class TrackState(C.Structure):
    """kfn_track_state (include/kfnet_hip.h): the record in device memory that carries the tracker from frame to frame."""
    _fields_ = [('committed', C.c_double * 12), ('estimate', C.c_double * 12), ('last_share', C.c_double), ('last_rms', C.c_double),
                ('last_pairs', C.c_double), ('frame', C.c_int32), ('lost', C.c_int32), ('accepted', C.c_int32),
                ('iterations', C.c_int32)]


TRACK_SUMS, TRACK_SUMS_LD, TRACK_TRAJ_LD, TRACK_ICP_BLOCK = 29, 32, 20, 1024


class RelocDesc(SizedStructure):
    """kfn_reloc_desc (include/kfnet_hip.h); `struct_size` is filled in here.  kfnet_amd.track.Relocaliser derives it."""
    _fields_ = ([(n, C.c_int32) for n in ('struct_size', 'H', 'W', 'levels', 'reloc_level', 'ferns', 'capacity', 'tries', 'harvest',
                                          'rows', 'traj_rows', 'slot', 'first', 'colour')] +
                [(n, C.c_float) for n in ('reloc_min_share', 'reloc_max_rms')])


class RelocState(C.Structure):
    """kfn_reloc_state (include/kfnet_hip.h): the record in device memory that carries the relocaliser from frame to frame."""
    _fields_ = ([('anchor', C.c_double * 12)] +
                [(n, C.c_int32) for n in ('n', 'streak', 'seeded', 'seed_key', 'candidates', 'min_d', 'recovered', 'reserved')] +
                [('cand_d', C.c_int32 * 4), ('cand_index', C.c_int32 * 4)])


RELOC_ROW_LD, RELOC_MAX_FERNS, RELOC_MAX_CAPACITY, RELOC_MAX_TRIES = 8, 4096, 65536, 4


class FilterLossDesc(SizedStructure):
    """kfn_filter_loss_desc (include/kfnet_hip.h); `struct_size` is filled in here."""
    _fields_ = [('struct_size', C.c_int32), ('B', C.c_int32), ('h', C.c_int32), ('w', C.c_int32), ('ld_pred', C.c_int32),
                ('ld_dpred', C.c_int32), ('label_stride', C.c_int32), ('img_stride', C.c_int32),
                ('has_transform', C.c_int32), ('transform', C.c_float * 12), ('has_loss_clip', C.c_int32),
                ('loss_clip', C.c_float), ('smooth_weight', C.c_float), ('weight_measure', C.c_float),
                ('weight_temporal', C.c_float), ('weight_kf', C.c_float), ('dist_threshold', C.c_double),
                ('min_uncertainty', C.c_double)]


class FilterBackwardDesc(SizedStructure):
    """kfn_filter_backward_desc (include/kfnet_hip.h); `struct_size` is filled in here."""
    _fields_ = ([(n, C.c_int32) for n in ('struct_size', 'S', 'T', 'H', 'W', 'ld_dpred', 'radius', 'reserved')] +
                [('min_uncertainty', C.c_double)])


class FlowLossDesc(SizedStructure):
    """kfn_flow_loss_desc (include/kfnet_hip.h); `struct_size` is filled in here."""
    _fields_ = [('struct_size', C.c_int32), ('P', C.c_int32), ('h', C.c_int32), ('w', C.c_int32), ('label_stride', C.c_int32),
                ('has_loss_clip', C.c_int32), ('loss_clip', C.c_float), ('reserved', C.c_int32),
                ('dist_threshold', C.c_double), ('min_uncertainty', C.c_double)]


REPROJ_MAX_OUTPUTS = 3


class ReprojOutput(C.Structure):
    """kfn_reproj_output (include/kfnet_hip.h)."""
    _fields_ = [('x', C.c_void_p), ('dx', C.c_void_p), ('weight', C.c_float), ('ld_x', C.c_int32), ('ld_dx', C.c_int32),
                ('reserved', C.c_int32)]


class ReprojDesc(SizedStructure):
    """kfn_reproj_desc (include/kfnet_hip.h); `struct_size` is filled in here.  kfnet_amd.reproj.descriptor derives it."""
    _fields_ = ([(n, C.c_int32) for n in ('struct_size', 'B', 'h', 'w', 'label_stride', 'outputs')] +
                [(n, C.c_float) for n in ('u', 'v', 'inv_fx', 'inv_fy')] + [('out', ReprojOutput * REPROJ_MAX_OUTPUTS)])


class LossScaleState(C.Structure):
    """kfn_loss_scale_state (include/kfnet_hip.h): the record in device memory that drives dynamic loss scaling."""
    _fields_ = [('beta1_power', C.c_double), ('beta2_power', C.c_double), ('scale', C.c_float), ('good_steps', C.c_int32),
                ('overflow', C.c_int32), ('skipped', C.c_int32), ('adam_t', C.c_int32), ('reserved', C.c_int32)]


# name -> (restype, argtypes); every symbol declared in include/kfnet_hip.h
_vp, _i, _sz = C.c_void_p, C.c_int, C.c_size_t
SYMBOLS = {
    'kfn_last_error': (C.c_char_p, []),
    'kfn_abi_version': (_i, []),
    'kfn_device_info': (_i, [_i, C.POINTER(_i), C.POINTER(_i), C.c_char_p, _i]),
    'kfn_malloc': (_i, [C.POINTER(_vp), _sz]),
    'kfn_free': (_i, [_vp]),
    'kfn_memcpy_h2d': (_i, [_vp, _vp, _sz, _vp]),
    'kfn_memcpy_d2h': (_i, [_vp, _vp, _sz, _vp]),
    'kfn_memcpy_d2d': (_i, [_vp, _vp, _sz, _vp]),
    'kfn_memset': (_i, [_vp, _i, _sz, _vp]),
    'kfn_stream_create': (_i, [C.POINTER(_vp)]),
    'kfn_stream_destroy': (_i, [_vp]),
    'kfn_stream_sync': (_i, [_vp]),
    'kfn_event_create': (_i, [C.POINTER(_vp)]),
    'kfn_event_destroy': (_i, [_vp]),
    'kfn_event_record': (_i, [_vp, _vp]),
    'kfn_event_elapsed_ms': (_i, [_vp, _vp, C.POINTER(C.c_float)]),
    'kfn_conv2d_nhwc': (_i, [C.POINTER(ConvDesc), _vp, _vp, _vp, _vp, _vp]),
    'kfn_conv2d_out_shape': (_i, [C.POINTER(ConvDesc), C.POINTER(_i), C.POINTER(_i)]),
    'kfn_conv2d_plan': (_i, [C.POINTER(ConvDesc), C.POINTER(_i), C.POINTER(_i), C.POINTER(_i)]),
    'kfn_winograd_plan': (_i, [C.POINTER(ConvDesc), C.POINTER(_i), C.POINTER(_i), C.POINTER(_i)]),
    'kfn_winograd_workspace_bytes': (_i, [C.POINTER(ConvDesc), C.POINTER(_sz)]),
    'kfn_conv2d_winograd': (_i, [C.POINTER(ConvDesc), _vp, _vp, _vp, _vp, _vp, _i, _vp]),
    'kfn_conv2d_winograd_fused': (_i, [C.POINTER(ConvDesc), _vp, _vp, _vp, _vp, _vp]),
    'kfn_winograd_fused_supported': (_i, [C.POINTER(ConvDesc)]),
    'kfn_conv2d_winograd_s2': (_i, [C.POINTER(ConvDesc), _vp, _vp, _vp, _vp, _vp]),
    'kfn_winograd_s2_supported': (_i, [C.POINTER(ConvDesc)]),
    'kfn_winograd_s2_splitk_workspace_bytes': (_i, [C.POINTER(ConvDesc), _i, C.POINTER(_sz)]),
    'kfn_conv2d_winograd_s2_splitk': (_i, [C.POINTER(ConvDesc), _vp, _vp, _vp, _vp, _vp, _i, _vp]),
    'kfn_conv2d_winograd_f43': (_i, [C.POINTER(ConvDesc), _vp, _vp, _vp, _vp, _vp]),
    'kfn_winograd_f43_supported': (_i, [C.POINTER(ConvDesc)]),
    'kfn_winograd_lds_bytes': (_i, [C.POINTER(ConvDesc), C.POINTER(_i)]),
    'kfn_winograd_launch_plan': (_i, [C.POINTER(ConvDesc), _i, _i, C.c_uint, C.POINTER(WinoPlan)]),
    'kfn_winograd_f43_splitk_workspace_bytes': (_i, [C.POINTER(ConvDesc), _i, C.POINTER(_sz)]),
    'kfn_conv2d_winograd_f43_splitk': (_i, [C.POINTER(ConvDesc), _vp, _vp, _vp, _vp, _vp, _i, _vp]),
    'kfn_conv3x3_c64_f16': (_i, [C.POINTER(ConvDesc), _vp, _vp, _vp, _vp, _vp]),
    'kfn_conv3x3_c64_f16_supported': (_i, [C.POINTER(ConvDesc)]),
    'kfn_first_conv_u8': (_i, [_vp, _i, _i, _i, _vp, _vp, _vp, _i, _vp, _vp, _vp, _i, _vp]),
    'kfn_first_conv_u8_ex': (_i, [_vp, _i, _i, _i, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _i, _vp]),
    'kfn_cost_volume': (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _vp]),
    'kfn_cost_volume_conv': (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _vp]),
    'kfn_pad_nhwc': (_i, [_vp, _vp, _i, _i, _i, _i, _i, _vp]),
    'kfn_cost_volume_gather': (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp]),
    'kfn_flow_softargmax': (_i, [_vp, _vp, _vp, _i, _i, _vp]),
    'kfn_flow_head': (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _vp]),
    'kfn_oflow_tail': (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp]),
    'kfn_oflow_head': (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp]),
    'kfn_oflow_head_f16': (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp]),
    'kfn_oflow_tail2': (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    'kfn_oflow_tail2_f16': (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    'kfn_kalman_scan_scratch_bytes': (_i, [C.POINTER(KalmanDesc), C.POINTER(_sz)]),
    'kfn_kalman_scan_plan': (_i, [C.POINTER(KalmanDesc), _i, C.POINTER(_i), C.POINTER(_i), C.POINTER(_i)]),
    'kfn_kalman_scan': (_i, [C.POINTER(KalmanDesc), _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    'kfn_kalman_scan_ex': (_i, [C.POINTER(KalmanDesc), _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp, _vp]),
    'kfn_eval_metrics': (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, C.c_double, C.c_double, _vp, _vp, _vp]),
    'kfn_kalman_fuse': (_i, [_vp, _vp, _vp, _vp, C.c_long, _vp]),
    'kfn_kalman_arith_probe': (_i, [_vp, _vp, _vp, C.c_long, _vp]),
    'kfn_kalman_fuse2': (_i, [_vp, _vp, _vp, C.c_long, _vp]),
    'kfn_copy_channels': (_i, [_vp, _i, _vp, _i, _i, _i, _vp]),
    'kfn_apply_transform': (_i, [_vp, _i, _vp, _i, _i, _i, _i, _vp, _i, _vp]),
    'kfn_pixel_map': (_i, [_vp, _i, _i, _i, _i, _i, C.c_float, C.c_float, C.c_float, C.c_float, _vp]),
    'kfn_bilinear_sampler': (_i, [_vp, _i, _i, _i, _i, _i, _vp, _i, _i, _i, _vp, _i, _vp]),
    'kfn_coord_records': (_i, [_vp, _i, _vp, _vp, C.c_long, _vp]),
    'kfn_flow_records': (_i, [_vp, _vp, _vp, C.c_long, _vp]),
    'kfn_decode_png_rgb8': (_i, [C.POINTER(C.c_char_p), _i, _i, _i, _vp, C.POINTER(_i), _i]),
    'kfn_crc32c': (_i, [_vp, _sz, C.POINTER(C.c_uint32)]),
    'kfn_pnp_scratch_bytes': (_i, [C.POINTER(PnPDesc), C.POINTER(_sz)]),
    'kfn_pnp_ransac': (_i, [C.POINTER(PnPDesc), _vp, _vp, _vp, _vp, _vp]),
    'kfn_pnp_hypotheses': (_i, [C.POINTER(PnPDesc), _vp, _vp, _vp, _vp, _vp]),
    'kfn_comm_available': (_i, []),
    'kfn_comm_unique_id': (_i, [_vp, _sz]),
    'kfn_comm_init': (_i, [C.POINTER(_vp), _i, _i, _vp, _i]),
    'kfn_comm_destroy': (_i, [_vp]),
    'kfn_comm_rank': (_i, [_vp, C.POINTER(_i), C.POINTER(_i)]),
    'kfn_send_state': (_i, [_vp, _i, _vp, _i, _i, _vp]),
    'kfn_recv_state': (_i, [_vp, _i, _vp, _i, _i, _vp]),
    # training SCoordNet (added exports, ABI 12)
    'kfn_conv2d_grad_weights_workspace_bytes': (_i, [C.POINTER(ConvDesc), C.POINTER(_sz)]),
    'kfn_conv2d_grad_weights_plan': (_i, [C.POINTER(ConvDesc), C.POINTER(_i), C.POINTER(_i), C.POINTER(_i), C.POINTER(_i),
                                          C.POINTER(C.c_long)]),
    'kfn_conv2d_grad_weights': (_i, [C.POINTER(ConvDesc), _vp, _vp, _vp, _vp, _vp, _vp]),
    'kfn_first_conv_u8_grad_weights_workspace_bytes': (_i, [_i, _i, _i, _i, C.POINTER(_sz)]),
    'kfn_first_conv_u8_grad_weights': (_i, [_vp, _i, _i, _i, _vp, _i, _vp, _vp, _vp, _vp]),
    'kfn_relu_grad': (_i, [_vp, _i, _vp, _i, C.c_long, _i, _vp]),
    'kfn_pack_conv_weights_floats': (_i, [_i, _i, _i, _i, _i, C.POINTER(_sz)]),
    'kfn_pack_conv_weights': (_i, [_vp, _i, _i, _i, _i, _i, _vp, _vp]),
    'kfn_coord_loss_grad': (_i, [C.POINTER(CoordLossDesc), _vp, _vp, _vp, _vp, _vp, _vp]),
    'kfn_adam_step': (_i, [_vp, _vp, _vp, _vp, C.c_long, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, _vp]),
    # augmenting a training batch (added exports, ABI 13)
    'kfn_frame_channel_sums': (_i, [_vp, _i, _i, _i, _vp, _vp]),
    'kfn_augment_batch': (_i, [C.POINTER(AugmentDesc), _vp, _vp, _vp, _vp, _vp, _vp]),
    # training labels from depth maps and poses (added exports, ABI 13)
    'kfn_decode_png_gray16': (_i, [C.POINTER(C.c_char_p), _i, _i, _i, _vp, C.POINTER(_i), _i]),
    'kfn_depth_labels': (_i, [C.POINTER(DepthLabelsDesc), _vp, _vp, _vp, _vp]),
    'kfn_label_moments': (_i, [C.POINTER(LabelMomentsDesc), _vp, _vp, _vp]),
    # fine-tuning SCoordNet through the Kalman filter (added exports, ABI 13)
    'kfn_measurement_map': (_i, [_vp, _i, _vp, C.c_long, _vp]),
    'kfn_filter_loss_grad': (_i, [C.POINTER(FilterLossDesc), _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    'kfn_filter_backward_scratch_bytes': (_i, [C.POINTER(FilterBackwardDesc), C.POINTER(_sz)]),
    'kfn_filter_backward': (_i, [C.POINTER(FilterBackwardDesc), _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    # training OFlowNet (added exports, ABI 13)
    'kfn_cost_volume_backward': (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    'kfn_flow_head_backward': (_i, [_vp, _vp, _vp, _vp, _vp, _i, _vp, _i, C.c_long, _vp]),
    'kfn_l2norm_backward': (_i, [_vp, _i, _vp, _i, _vp, _i, C.c_long, _i, _vp]),
    'kfn_flow_loss_grad': (_i, [C.POINTER(FlowLossDesc), _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    # joint stage 3: both networks through the Kalman filter (added export, ABI 13)
    'kfn_filter_backward_joint': (_i, [C.POINTER(FilterBackwardDesc)] + [_vp] * 13),
    # mixed-precision training of SCoordNet (added exports, ABI 13)
    'kfn_pack_conv_weights_f16': (_i, [_vp, _i, _i, _i, _i, _i, _vp, _vp]),
    'kfn_loss_scale_apply': (_i, [_vp, C.c_long, _vp, _vp]),
    'kfn_loss_scale_unscale_check': (_i, [_vp, C.c_long, _vp, _vp]),
    'kfn_adam_step_guarded': (_i, [_vp, _vp, _vp, _vp, C.c_long, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, _i,
                               _vp, _vp]),
    # uncertainty-aware poses: weighted refinement, pose covariance, pose filter (added exports, ABI 13)
    'kfn_pnp_ransac_unc': (_i, [C.POINTER(PnPDesc), C.POINTER(PnPUncDesc), _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    'kfn_pose_filter': (_i, [C.POINTER(PoseFilterDesc), _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    # the pose tracker: motion models, backward pass, carried state (added exports, ABI 13)
    'kfn_pose_track_state_bytes': (_i, [C.POINTER(PoseTrackDesc), C.POINTER(_sz)]),
    'kfn_pose_track_scratch_bytes': (_i, [C.POINTER(PoseTrackDesc), C.POINTER(_sz)]),
    'kfn_pose_track': (_i, [C.POINTER(PoseTrackDesc)] + [_vp] * 11),
    # the reprojection loss for stages 1 and 3, with the augmented pixel map (added exports, ABI 13)
    'kfn_reproj_loss_grad': (_i, [C.POINTER(ReprojDesc), _vp, _vp, _vp, _vp, _i, _vp, _vp]),
    'kfn_augment_pixel_map': (_i, [C.POINTER(AugmentDesc), C.c_float, C.c_float, C.c_float, C.c_float, _vp, _vp]),
    # guided sampling: hypotheses drawn by the maps' confidence (added exports, ABI 13)
    'kfn_pnp_guided_scratch_bytes': (_i, [C.POINTER(PnPDesc), C.POINTER(PnPSampleDesc), C.POINTER(_sz)]),
    'kfn_pnp_ransac_guided': (_i, [C.POINTER(PnPDesc), C.POINTER(PnPSampleDesc), C.POINTER(PnPUncDesc)] + [_vp] * 7),
    'kfn_pnp_hypotheses_guided': (_i, [C.POINTER(PnPDesc), C.POINTER(PnPSampleDesc)] + [_vp] * 8),
    # labels, depth maps and frames rendered from a triangle mesh (added exports, ABI 13)
    'kfn_render_scratch_bytes': (_i, [C.POINTER(RenderDesc), C.POINTER(_sz)]),
    'kfn_render': (_i, [C.POINTER(RenderDesc)] + [_vp] * 10),
    # depth maps fused into a TSDF volume, and the scene mesh extracted from it (added exports, ABI 13)
    'kfn_fuse_scratch_bytes': (_i, [C.POINTER(FuseDesc), C.POINTER(_sz)]),
    'kfn_fuse_integrate': (_i, [C.POINTER(FuseDesc)] + [_vp] * 6),
    'kfn_fuse_extract_count': (_i, [C.POINTER(FuseDesc), _vp, _vp, _vp, _vp]),
    'kfn_fuse_extract': (_i, [C.POINTER(FuseDesc)] + [_vp] * 6 + [C.c_int64, C.c_int64, _vp]),
    # the camera tracked against the TSDF volume: live maps, ray cast, ICP sums, solve, commit (added exports, ABI 13)
    'kfn_track_scratch_bytes': (_i, [C.POINTER(TrackDesc), C.POINTER(_sz)]),
    'kfn_track_live_maps': (_i, [C.POINTER(TrackDesc)] + [_vp] * 4),
    'kfn_track_raycast': (_i, [C.POINTER(TrackDesc)] + [_vp] * 5),
    'kfn_track_icp_sums': (_i, [C.POINTER(TrackDesc)] + [_vp] * 8),
    'kfn_track_update': (_i, [C.POINTER(TrackDesc)] + [_vp] * 3),
    'kfn_track_commit': (_i, [C.POINTER(TrackDesc)] + [_vp] * 4),
    # a lost tracker relocalised from fern-coded keyframes: encode, search, seed, settle (added exports, ABI 13)
    'kfn_reloc_encode': (_i, [C.POINTER(RelocDesc)] + [_vp] * 5),
    'kfn_reloc_search': (_i, [C.POINTER(RelocDesc)] + [_vp] * 5),
    'kfn_reloc_seed': (_i, [C.POINTER(RelocDesc)] + [_vp] * 4),
    'kfn_reloc_settle': (_i, [C.POINTER(RelocDesc)] + [_vp] * 9),
    # poses from the records and a depth frame: RANSAC-Kabsch (added exports, ABI 13)
    'kfn_kabsch_scratch_bytes': (_i, [C.POINTER(KabschDesc), C.POINTER(_sz)]),
    'kfn_kabsch_ransac': (_i, [C.POINTER(KabschDesc)] + [_vp] * 8),
    'kfn_kabsch_hypotheses': (_i, [C.POINTER(KabschDesc)] + [_vp] * 6),
    'kfn_kabsch_select': (_i, [_vp, _i, _i, _vp, _vp]),
}

_lib = None


def load():
    """Load the HIP library (once).  Fails loudly: there is no fallback path."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise KfnError('%s not found -- run `python -m kfnet_amd.build` (hipcc, gfx950); '
                       'kfnet_amd has no CPU fallback' % LIB_PATH)
    try:
        # torch bundles its own libamdhip64; the library must bind to that runtime, not to a second copy from
        # /opt/rocm, or torch's device pointers mean nothing to it ("no ROCm-capable device is detected")
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is missing
        fn.restype = res
        fn.argtypes = args
    if lib.kfn_abi_version() != ABI_VERSION:
        raise KfnError('libkfnet_hip.so ABI version mismatch')
    _lib = lib
    return lib


def check(rc, what=''):
    if rc != KFN_OK:
        msg = load().kfn_last_error()
        raise KfnError('%s failed (%d): %s' % (what, rc, msg.decode() if msg else '?'))
