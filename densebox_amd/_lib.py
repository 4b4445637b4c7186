"""ctypes binding of libdensebox_hip.so (the C ABI declared in include/densebox_hip.h).

The library must be present (built in-tree by ``densebox_amd._build`` /
``__graft_entry__.build()``); there is no fallback -- a missing library raises.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# DBX_LIB: load another build of the same library (tools/build_variant.sh makes same-box A/B builds of one source file)
LIB_PATH = os.environ.get('DBX_LIB') or os.path.join(_HERE, 'csrc', 'libdensebox_hip.so')

F16, BF16, F32 = 0, 1, 2
DTYPE_ID = {'f16': F16, 'bf16': BF16, 'f32': F32}
ESIZE = {F16: 2, BF16: 2, F32: 4}

EPI_BIAS, EPI_RELU, EPI_GATE, EPI_DROPMASK, EPI_ACCUM, EPI_F32_NCHW, EPI_DROPHASH = 1, 2, 4, 8, 16, 32, 64
CONV_WFRAG = 128          # w_packed is in MFMA-fragment order (pack modes 4/5)
K_IGEMM, K_DMA, K_BAND, K_C64, K_C8, K_WS, K_P8 = 1, 2, 3, 4, 5, 6, 7


class View(C.Structure):
    _fields_ = [('ptr', C.c_void_p), ('n', C.c_int32), ('h', C.c_int32), ('w', C.c_int32),
                ('pad', C.c_int32), ('ld', C.c_int32), ('c_off', C.c_int32), ('c', C.c_int32)]


class ConvDesc(C.Structure):
    _fields_ = [('dtype', C.c_int32), ('kh', C.c_int32), ('kw', C.c_int32), ('cpad', C.c_int32),
                ('cin_pad', C.c_int32), ('cout_pad', C.c_int32), ('epilogue', C.c_int32), ('drop_seed', C.c_uint32)]


class ConvPlan(C.Structure):
    _fields_ = [('kernel', C.c_int32), ('tile_m', C.c_int32), ('tile_n', C.c_int32), ('w_frag', C.c_int32),
                ('name', C.c_char * 64)]


class Head2UpHalf(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ('px_lo', 'px_n', 'own_lo', 'own_hi', 'ix_lo', 'ix_n')]


class Head2UpLaunch(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ('head0', 'heads', 'kj', 'groups', 'blocks')]


class Head2UpPlan(C.Structure):
    _fields_ = [('fused', C.c_int32), ('halves', C.c_int32), ('half', Head2UpHalf * 2), ('launches', C.c_int32),
                ('launch', Head2UpLaunch * 4)]


class UpsampleBwdPlan(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ('kernel', 'nseg', 'workgroups', 'lds_bytes')]


class LossDesc(C.Structure):
    _fields_ = [('kind', C.c_int32), ('n', C.c_int32), ('half_neg', C.c_int32),
                ('lambda_loc', C.c_float), ('lambda_det', C.c_float), ('lambda_lm', C.c_float),
                ('use_labels', C.c_int32)]


class LossIO(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in (
        'bbox', 'vertices', 'labels', 'rand_neg', 'lm_rand_neg',
        'score', 'loc', 'lm', 'rf', 'lmloc',
        'd_score', 'd_loc', 'd_lm', 'd_rf', 'd_lmloc',
        'loss', 'mask_cls', 'mask_lm', 'neg_idx', 'lm_neg_idx', 'pos_count')]


class WarpJob(C.Structure):
    _fields_ = [('src', C.c_void_p), ('sh', C.c_int32), ('sw', C.c_int32), ('m9', C.c_double * 9), ('dh', C.c_int32),
                ('dw', C.c_int32), ('x0', C.c_int32), ('y0', C.c_int32), ('oh', C.c_int32), ('ow', C.c_int32),
                ('dst_off', C.c_int64)]


class CropFrame(C.Structure):
    _fields_ = [('src', C.c_void_p), ('sh', C.c_int32), ('sw', C.c_int32)]


class EvalRecord(C.Structure):
    _fields_ = [('score', C.c_double), ('lm_err', C.c_double), ('status', C.c_int32), ('frame', C.c_int32)]


class Track(C.Structure):
    _fields_ = [('box', C.c_double * 4), ('vel', C.c_double * 4), ('score', C.c_double), ('best_score', C.c_double), ('id', C.c_int32),
                ('hits', C.c_int32), ('age', C.c_int32), ('first_frame', C.c_int32), ('last_frame', C.c_int32), ('best_frame', C.c_int32)]


class TrackRecord(C.Structure):
    _fields_ = [('stream', C.c_int32), ('reserved', C.c_int32), ('t', Track)]


class Shot(C.Structure):
    _fields_ = [('key', C.c_double), ('score', C.c_double), ('sharpness', C.c_int64), ('id', C.c_int32), ('frame', C.c_int32),
                ('shots', C.c_int32), ('reserved', C.c_int32)]


class ShotRecord(C.Structure):
    _fields_ = [('stream', C.c_int32), ('slot', C.c_int32), ('shot', Shot)]


class ZoneLine(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ('ax', 'ay', 'bx', 'by')]


class ZonePoly(C.Structure):
    _fields_ = [('n', C.c_int32), ('role', C.c_int32), ('xy', C.c_int32 * 32)]


class ZoneConfig(C.Structure):
    _fields_ = [('n_lines', C.c_int32), ('n_regions', C.c_int32), ('n_masks', C.c_int32), ('reserved', C.c_int32),
                ('lines', ZoneLine * 8), ('regions', ZonePoly * 8), ('masks', ZonePoly * 8)]


class ZoneState(C.Structure):
    _fields_ = [('owner_id', C.c_int32), ('has_prev', C.c_int32), ('px', C.c_int32), ('py', C.c_int32), ('inside', C.c_int32),
                ('reserved', C.c_int32 * 3)]


class ZoneEvent(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ('stream', 'track_id', 'kind', 'index', 'frame', 'hits', 'ax', 'ay')]


class OverlayFrame(C.Structure):
    _fields_ = [('src', C.c_void_p), ('dst', C.c_void_p), ('h', C.c_int32), ('w', C.c_int32)]


class OverlayStyle(C.Structure):
    _fields_ = [('box_color', C.c_uint8 * 4), ('text_color', C.c_uint8 * 4), ('mark_color', C.c_uint8 * 4), ('thickness', C.c_int32),
                ('radius', C.c_int32), ('font_scale', C.c_int32), ('inset_scale', C.c_int32)]


class RedactStyle(C.Structure):
    _fields_ = [('color', C.c_uint8 * 4), ('method', C.c_int32), ('shape', C.c_int32), ('cell', C.c_int32), ('radius', C.c_int32),
                ('grow', C.c_int32), ('grow_pct', C.c_int32), ('coast', C.c_int32), ('min_score', C.c_double)]


class ResizeJob(C.Structure):
    _fields_ = [('src', C.c_void_p), ('sh', C.c_int32), ('sw', C.c_int32), ('cx0', C.c_int32), ('cy0', C.c_int32),
                ('cw', C.c_int32), ('ch', C.c_int32), ('pad_l', C.c_int32), ('pad_t', C.c_int32), ('pad_r', C.c_int32),
                ('pad_b', C.c_int32), ('pad_value', C.c_int32), ('dh', C.c_int32), ('dw', C.c_int32), ('dst_off', C.c_int64)]


class Nv12Frame(C.Structure):
    _fields_ = [('y', C.c_void_p), ('uv', C.c_void_p), ('rgb', C.c_void_p), ('h', C.c_int32), ('w', C.c_int32), ('pitch_y', C.c_int32),
                ('pitch_uv', C.c_int32), ('pitch_rgb', C.c_int32), ('reserved', C.c_int32)]


class Nv12Params(C.Structure):
    _fields_ = [('standard', C.c_int32), ('range', C.c_int32), ('order', C.c_int32), ('reserved', C.c_int32)]


class ResizeJobNv12(C.Structure):
    _fields_ = [('y', C.c_void_p), ('uv', C.c_void_p), ('pitch_y', C.c_int32), ('pitch_uv', C.c_int32), ('sh', C.c_int32),
                ('sw', C.c_int32), ('cx0', C.c_int32), ('cy0', C.c_int32), ('cw', C.c_int32), ('ch', C.c_int32), ('pad_l', C.c_int32),
                ('pad_t', C.c_int32), ('pad_r', C.c_int32), ('pad_b', C.c_int32), ('pad_value', C.c_int32), ('dh', C.c_int32),
                ('dw', C.c_int32), ('dst_off', C.c_int64)]


class PatchJob(C.Structure):
    _fields_ = [('src', C.c_void_p), ('dst', C.c_void_p), ('scale_x', C.c_double), ('scale_y', C.c_double), ('row_bytes', C.c_int32),
                ('cx0', C.c_int32), ('cy0', C.c_int32), ('cw', C.c_int32), ('ch', C.c_int32), ('pad_l', C.c_int32), ('pad_t', C.c_int32),
                ('vw', C.c_int32), ('vh', C.c_int32), ('dh', C.c_int32), ('dw', C.c_int32), ('pad_value', C.c_int32),
                ('tiles_x', C.c_int32), ('frame', C.c_int32), ('kind', C.c_int32), ('reserved', C.c_int32)]


class PatchGeom(C.Structure):
    _fields_ = [('status', C.c_int32), ('x0', C.c_int32), ('y0', C.c_int32), ('x1', C.c_int32), ('y1', C.c_int32),
                ('labels', C.c_int32 * 12), ('reserved', C.c_int32)]


class PatchPlanIO(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in (
        'frames', 'plates', 'plate0', 'cand', 'draws', 'state', 'jobs', 'labels', 'bbox', 'vertices', 'label', 'count', 'tally',
        'status', 'slot', 'cand_out', 'draws_out')]


class PatchAug(C.Structure):
    _fields_ = [('flags', C.c_int32), ('blur', C.c_int32), ('box_len', C.c_int32), ('sat', C.c_int32), ('contrast', C.c_int32),
                ('brightness', C.c_int32), ('curve', C.c_int32), ('noise_amp', C.c_int32), ('key_lo', C.c_int32), ('key_hi', C.c_int32),
                ('gain', C.c_int32 * 3), ('reserved', C.c_int32 * 3)]


class PatchAugCfg(C.Structure):
    _fields_ = [('p_flip', C.c_double), ('p_blur', C.c_double), ('p_curve', C.c_double), ('p_noise', C.c_double), ('kind_w', C.c_int32 * 3),
                ('box_lo', C.c_int32), ('box_hi', C.c_int32), ('sat_lo', C.c_int32), ('sat_hi', C.c_int32), ('contrast_lo', C.c_int32),
                ('contrast_hi', C.c_int32), ('brightness_lo', C.c_int32), ('brightness_hi', C.c_int32), ('gain_lo', C.c_int32),
                ('gain_hi', C.c_int32), ('noise_lo', C.c_int32), ('noise_hi', C.c_int32), ('curve_lo', C.c_int32), ('curve_hi', C.c_int32),
                ('G', C.c_int32), ('reserved', C.c_int32 * 2)]


class PatchAugIO(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ('labels_in', 'count', 'params_in', 'state', 'params', 'labels', 'bbox', 'vertices', 'label')]


class PatchWarpRec(C.Structure):
    _fields_ = [('flags', C.c_int32), ('border', C.c_int32), ('fill', C.c_int32), ('rot', C.c_int32), ('quad', C.c_int32 * 8),
                ('scale', C.c_int32), ('aspect', C.c_int32), ('shear', C.c_int32), ('reserved', C.c_int32)]


class PatchWarpCfg(C.Structure):
    _fields_ = [('p_warp', C.c_double), ('rot_lo', C.c_int32), ('rot_hi', C.c_int32), ('scale_lo', C.c_int32), ('scale_hi', C.c_int32),
                ('aspect_lo', C.c_int32), ('aspect_hi', C.c_int32), ('shear_lo', C.c_int32), ('shear_hi', C.c_int32), ('tx', C.c_int32),
                ('ty', C.c_int32), ('jitter', C.c_int32), ('margin', C.c_int32), ('border', C.c_int32), ('fill', C.c_int32), ('R', C.c_int32),
                ('reserved', C.c_int32)]


class PatchWarpIO(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ('labels_in', 'count', 'params_in', 'state', 'rot', 'params', 'labels', 'bbox', 'vertices', 'label',
                                          'fwd', 'inv')]


class MergeXform(C.Structure):
    _fields_ = [('scale', C.c_double), ('off_x', C.c_double), ('off_y', C.c_double)]


class Tile(C.Structure):
    _fields_ = [('frame', C.c_int32), ('x0', C.c_int32), ('y0', C.c_int32), ('side', C.c_int32), ('cw', C.c_int32), ('ch', C.c_int32),
                ('scale', C.c_double), ('lo2x', C.c_double), ('hi2x', C.c_double), ('lo2y', C.c_double), ('hi2y', C.c_double)]


TILE_RULE_NONE, TILE_RULE_CORE = 0, 1


_VP, _I32, _I64, _F, _D = C.c_void_p, C.c_int32, C.c_int64, C.c_float, C.c_double
_PV, _PC = C.POINTER(View), C.POINTER(ConvDesc)

# name -> (restype, argtypes).  Must list every symbol include/densebox_hip.h declares
# (tests/test_abi.py cross-checks this table against the header and the built library).
SIGNATURES = {
    'dbx_last_error': (C.c_char_p, []),
    'dbx_version': (C.c_int, []),
    'dbx_device_arch': (C.c_int, [C.c_int]),
    'dbx_conv_packed_elems': (_I64, [_PC]),
    'dbx_conv_forward': (C.c_int, [_PC, _PV, _VP, _VP, _PV, _PV, _VP, _I32, _VP]),
    'dbx_conv_plan': (C.c_int, [_PC, _PV, _PV, C.POINTER(ConvPlan)]),
    'dbx_conv_forward_split': (C.c_int, [_PC, _PV, _VP, _VP, _PV, _PV, _PV, _PV, _I32, _I32, _VP]),
    'dbx_heads_forward_fusable': (C.c_int, [_PC, _PV, _PV, C.POINTER(C.c_int32), _I32]),
    'dbx_heads_forward_fused_scratch_bytes': (_I64, [_I32, _I64]),
    'dbx_heads_forward_fused': (C.c_int, [_PC, _PV, _VP, _VP, _PV, _VP, _VP, C.POINTER(C.c_int32), _I32, _VP, _VP, _VP]),
    'dbx_heads_forward_fused_heads': (C.c_int, [_PC, _PV, _VP, _VP, _PV, _VP, _VP, C.POINTER(C.c_int32), _I32, C.POINTER(C.c_void_p), _VP, _VP]),
    'dbx_dp_unique_id': (C.c_int, [_VP]),
    'dbx_dp_init': (C.c_int, [_VP, _I32, _I32, C.POINTER(C.c_void_p)]),
    'dbx_dp_allreduce_sum_f32': (C.c_int, [_VP, _VP, _I64, _VP]),
    'dbx_dp_destroy': (C.c_int, [_VP]),
    'dbx_conv_dgrad_wgrad1_scratch_bytes': (_I64, []),
    'dbx_conv_dgrad_wgrad1_fusable': (C.c_int, [_PC, _PV, _PV, _PV]),
    'dbx_conv_dgrad_wgrad1': (C.c_int, [_PC, _PV, _VP, _PV, _PV, _I32, _VP, _VP, _VP, _I32, _VP]),
    'dbx_conv_pool_fusable': (C.c_int, [_PC, _PV, _PV]),
    'dbx_conv_forward_pool': (C.c_int, [_PC, _PV, _VP, _VP, _PV, _PV, _I32, _VP]),
    'dbx_conv_forward_pool_idx': (C.c_int, [_PC, _PV, _VP, _VP, _PV, _PV, _I32, _VP, _VP]),
    'dbx_pack_weight': (C.c_int, [_I32, _I32, _VP, _I32, _I32, _I32, _I32, _VP, _I32, _I32, _I32, _I32, _VP]),
    'dbx_fold_heads': (C.c_int, [_VP, _VP, _VP, _VP, _I32, _VP, _VP, _VP]),
    'dbx_fold_refine': (C.c_int, [_VP, _VP, _VP, _VP, _VP, _VP, _I32, _I32, _VP, _VP, _VP, _VP]),
    'dbx_refine_eval': (C.c_int, [_VP, _VP, _I32, _I32, _I32, _VP, _VP, _VP, _VP]),
    'dbx_refine_backward_scratch_bytes': (C.c_int64, [_I32, _I32, _I32]),
    'dbx_refine_backward': (C.c_int, [_VP, _VP, _VP, _I32, _I32, _I32, _VP, _VP, _VP, _VP, _VP, _VP, _I32, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    'dbx_upsample_bilinear_nchw_f32': (C.c_int, [_VP, _I32, _I32, _I32, _VP, _I32, _I32, _VP]),
    'dbx_pack_multi': (C.c_int, [_I32, _VP, _I32, _I64, _VP]),
    'dbx_sgd_pack_step': (C.c_int, [_I32, _VP, _I32, _I64, _VP, _F, _F, _F, _I32, _VP]),
    'dbx_head2_dgrad': (C.c_int, [_I32, _PV, C.POINTER(C.c_void_p), C.POINTER(C.c_int32), _I32, _PV, _VP, _I32, _I32, C.c_uint32, _VP]),
    'dbx_head2_wgrad_scratch_bytes': (_I64, [_I32, _I32]),
    'dbx_head2_wgrad': (C.c_int, [_I32, _PV, _PV, C.POINTER(C.c_int32), _I32, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), _VP, _VP]),
    'dbx_head2_backward': (C.c_int, [_I32, _PV, _PV, C.POINTER(C.c_void_p), C.POINTER(C.c_int32), _I32, _PV, _VP, _I32, _I32, C.c_uint32,
                                     C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), _VP, _VP]),
    'dbx_head2_backward_up': (C.c_int, [_I32, _PV, _PV, C.POINTER(C.c_void_p), C.POINTER(C.c_int32), _I32, _PV, _VP, _I32, _I32, C.c_uint32,
                                        C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), _VP, _PV, _VP]),
    'dbx_perspective_matrix': (C.c_int, [_VP, _VP, _VP]),
    'dbx_warp_perspective_u8': (C.c_int, [_VP, _I32, _I32, _I32, _VP, _VP, _I32, _I32, _VP]),
    'dbx_warp_batch_workspace_bytes': (_I64, [_I32]),
    'dbx_warp_perspective_batch_u8': (C.c_int, [C.POINTER(WarpJob), _I32, _I32, _VP, _VP, _VP]),
    'dbx_plate_crops_batch': (C.c_int, [_VP, _I32, _I32, _VP, _I64, _I64, _VP, _I32, _I32, _I32, _VP, _VP, _VP, _VP]),
    'dbx_match_gt_batch': (C.c_int, [_VP, _I32, _I64, _VP, _VP, _I32, _I32, _VP, _I32, _VP, _VP, _I32, _D, _VP, _VP, _VP, _VP, _VP, _VP]),
    'dbx_eval_append': (C.c_int, [_VP, _I32, _I64, _VP, _VP, _I32, _I32, _VP, _VP, _VP, _VP, _I64, _VP, _VP]),
    'dbx_track_update_batch': (C.c_int, [_VP, _I32, _I64, _VP, _VP, _I32, _I32, _VP, _VP, _I32, _I32, _I32, _D, _I32, _D, _D, _D, _VP, _VP, _VP,
                                         _VP, _VP, _VP]),
    'dbx_track_append': (C.c_int, [_VP, _VP, _I32, _I32, _I32, _VP, _I64, _VP, _VP]),
    'dbx_crop_sharpness': (C.c_int, [_VP, _I64, _I32, _I32, _I32, _VP, _VP]),
    'dbx_track_gallery_update': (C.c_int, [_VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _I32, _I32, _I32, _I32, _I32, _I32,
                                           _I32, _I32, _I64, _I32, _D, _I32, _VP]),
    'dbx_draw_overlay_batch': (C.c_int, [_VP, _I32, _I32, _I32, _I32, _VP, _I32, _I64, _VP, _VP, _I32, _VP, _VP, _VP, _I32, _I32,
                                         C.POINTER(OverlayStyle), _VP]),
    'dbx_overlay_font': (C.c_int, [_VP]),
    'dbx_overlay_label': (C.c_int, [_D, _I32, C.c_char_p, _I32]),
    'dbx_redact_batch': (C.c_int, [_VP, _I32, _I32, _I32, _I32, _VP, _I32, _I64, _VP, _VP, _I32, _VP, _I32, _I32, _I32,
                                   C.POINTER(RedactStyle), _VP]),
    'dbx_redact_host': (C.c_int, [_VP, _VP, _I32, _I32, _I32, _VP, _I32, _I32, _VP, _I32, _VP, _I32, C.POINTER(RedactStyle)]),
    'dbx_zone_filter_keep': (C.c_int, [_VP, _I32, _I64, _VP, _VP, _I32, _I32, _VP, _I32, _I32, _I32, _VP, _VP, _VP]),
    'dbx_zone_update_batch': (C.c_int, [_VP, _VP, _VP, _VP, _VP, _VP, _I32, _I32, _I32, _I32, _I32, _I32, _VP, _VP, _I32, _VP]),
    'dbx_zone_append': (C.c_int, [_VP, _VP, _I32, _I32, _VP, _I64, _VP, _VP]),
    'dbx_zone_check_config': (C.c_int, [C.POINTER(ZoneConfig)]),
    'dbx_zone_host': (C.c_int, [_I32, _I64, _VP, _VP, _VP]),
    'dbx_resize_batch_workspace_bytes': (_I64, [_I32]),
    'dbx_resize_cubic_batch_u8': (C.c_int, [C.POINTER(ResizeJob), _I32, _I32, _VP, _VP, _VP]),
    'dbx_nv12_to_rgb_batch': (C.c_int, [_VP, _I32, _I32, _I32, C.POINTER(Nv12Params), _VP]),
    'dbx_rgb_to_nv12_batch': (C.c_int, [_VP, _I32, _I32, _I32, C.POINTER(Nv12Params), _VP]),
    'dbx_nv12_host': (C.c_int, [C.POINTER(Nv12Frame), C.POINTER(Nv12Params), _I32]),
    'dbx_resize_batch_nv12_workspace_bytes': (_I64, [_I32]),
    'dbx_resize_cubic_batch_nv12': (C.c_int, [C.POINTER(ResizeJobNv12), _I32, C.POINTER(Nv12Params), _VP, _VP, _VP]),
    'dbx_patch_plan': (C.c_int, [C.POINTER(PatchPlanIO), _I32, _I32, _I32, _I32, _I32, _D, _D, _I32, _VP]),
    'dbx_patch_cut': (C.c_int, [_VP, _VP, _I32, _I32, _VP, _VP]),
    'dbx_patch_plan_host': (C.c_int, [_I32, _I32, _I32, _VP, _I32, _D, _D, _D, _I32, C.POINTER(PatchGeom)]),
    'dbx_patch_draw': (C.c_int, [_I64, _I64, _I32, _I32, _VP]),
    'dbx_patch_check_tables': (C.c_int, [_VP, _I32, _VP, _I32, _VP, _I32]),
    'dbx_patch_aug_plan': (C.c_int, [C.POINTER(PatchAugIO), C.POINTER(PatchAugCfg), _I32, _VP]),
    'dbx_patch_augment': (C.c_int, [_VP, _VP, _VP, _VP, _I32, _I32, _I32, _VP, _VP]),
    'dbx_patch_aug_params_host': (C.c_int, [C.POINTER(PatchAugCfg), _I64, _I64, _VP, _VP, _I32, _VP, _VP, _VP, _VP, _VP]),
    'dbx_patch_augment_host': (C.c_int, [_VP, _VP, _VP, _I32, _I32, _VP]),
    'dbx_patch_warp_plan': (C.c_int, [C.POINTER(PatchWarpIO), C.POINTER(PatchWarpCfg), _I32, _VP]),
    'dbx_patch_warp': (C.c_int, [_VP, _VP, _VP, _VP, _I32, _I32, _VP, _VP]),
    'dbx_patch_warp_params_host': (C.c_int, [C.POINTER(PatchWarpCfg), _I64, _I64, _VP, _VP, _VP, _I32, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    'dbx_patch_warp_host': (C.c_int, [_VP, _VP, _VP, _I32, _VP]),
    'dbx_conv_wgrad_scratch_bytes': (_I64, [_I32, _PV, _PV, _I32, _I32]),
    'dbx_conv_wgrad': (C.c_int, [_I32, _PV, _PV, _I32, _I32, _I32, _I32, _I32, _VP, _VP, _VP, _I32, _VP]),
    'dbx_conv_wgrad_slice': (C.c_int, [_I32, _PV, _PV, _I32, _I32, _I32, _I32, _I32, _VP, _I32, _I32, _VP, _VP, _I32, _VP]),
    'dbx_conv_wgrad_pool_dz_ok': (C.c_int, [_I32, _PV, _PV, _I32, _I32]),
    'dbx_conv_wgrad_pool_dz': (C.c_int, [_I32, _PV, _VP, _I32, _PV, _PV, _I32, _I32, _I32, _I32, _I32, _VP, _VP, _VP, _I32, _I32, _VP]),
    'dbx_head2_backward_up_fused': (C.c_int, [_I32, _PV, _PV]),
    'dbx_head2_backward_up_plan': (C.c_int, [_I32, _PV, _PV, C.POINTER(C.c_int32), _I32, C.POINTER(Head2UpPlan)]),
    'dbx_heads1_wgrad_gen_ok': (C.c_int, [_I32, _PV, _I32]),
    'dbx_heads1_dgrad_gen': (C.c_int, [_I32, _PV, C.POINTER(C.c_void_p), C.POINTER(C.c_int32), _I32, _I32, C.c_uint32, _VP, _PV, _PV, _VP]),
    'dbx_heads1_wgrad_gen': (C.c_int, [_I32, _PV, _PV, C.POINTER(C.c_void_p), C.POINTER(C.c_int32), _I32, _I32, C.c_uint32, _I32, _VP, _I32, _I32,
                             _VP, _VP, _VP]),
    'dbx_conv_wgrad_plan': (C.c_int, [_I32, _PV, _PV, _I32, _I32, C.c_char_p, _I32, C.POINTER(C.c_int32)]),
    'dbx_nchw_to_framed': (C.c_int, [_I32, _VP, _I32, _PV, _VP]),
    'dbx_u8hwc_to_framed': (C.c_int, [_I32, _VP, _PV, C.POINTER(C.c_float), C.POINTER(C.c_float), _VP]),
    'dbx_nchw_to_framed_ch': (C.c_int, [_I32, _VP, _I32, _PV, _I32, _VP]),
    'dbx_nchw_to_framed_slots': (C.c_int, [_I32, _VP, _VP, _I32, _I32, _PV, _VP]),
    'dbx_framed_to_nchw_f32': (C.c_int, [_I32, _PV, _VP, _VP]),
    'dbx_framed_add_ch': (C.c_int, [_I32, _PV, _I32, _I32, _PV, _I32, _VP]),
    'dbx_maxpool2x2': (C.c_int, [_I32, _PV, _PV, _VP]),
    'dbx_maxpool2x2_bwd': (C.c_int, [_I32, _PV, _PV, _PV, _I32, _I32, _VP]),
    'dbx_maxpool_idx_bytes': (C.c_int64, [_I32, _I32, _I32, _I32]),
    'dbx_maxpool2x2_idx': (C.c_int, [_I32, _PV, _PV, _VP, _VP]),
    'dbx_maxpool2x2_bwd_idx': (C.c_int, [_I32, _VP, _PV, _PV, _I32, _I32, _VP]),
    'dbx_upsample_bilinear': (C.c_int, [_I32, _PV, _PV, _VP]),
    'dbx_upsample_bilinear_bwd': (C.c_int, [_I32, _PV, _PV, _PV, _VP]),
    'dbx_upsample_bilinear_bwd_plan': (C.c_int, [_I32, _PV, _PV, C.POINTER(UpsampleBwdPlan)]),
    'dbx_loss_scratch_bytes': (C.c_int64, [_I32]),
    'dbx_loss_forward_backward': (C.c_int, [C.POINTER(LossDesc), C.POINTER(LossIO), _VP, _VP]),
    'dbx_count_positives': (C.c_int, [_VP, _VP, _I32, _VP, _VP]),
    'dbx_init_score_map': (C.c_int, [_VP, _VP, _I32, _VP, _VP]),
    'dbx_init_offset_map': (C.c_int, [_VP, _VP, _I32, _I32, _VP, _VP]),
    'dbx_init_lm_heatmap': (C.c_int, [_VP, _VP, _I32, _I32, _VP, _VP]),
    'dbx_mask_by_sel': (C.c_int, [_VP, _I32, _VP, _I64, _VP, _I32, _VP]),
    'dbx_mask_gray_zone_cls': (C.c_int, [_VP, _VP, _VP, _I32, _VP]),
    'dbx_mask_gray_zone_lm': (C.c_int, [_VP, _I32, _VP, _I64, _VP]),
    'dbx_sgd_step': (C.c_int, [_VP, _VP, _I32, _I64, _F, _F, _F, _I32, _VP]),
    'dbx_grad_guard': (C.c_int, [_VP, _I64, _VP, _I32, _VP]),
    'dbx_sgd_step_guarded': (C.c_int, [_VP, _VP, _I32, _I64, _F, _F, _F, _I32, _VP, _I32, _VP]),
    'dbx_sgd_pack_step_guarded': (C.c_int, [_I32, _VP, _I32, _I64, _VP, _F, _F, _F, _I32, _VP, _I32, _VP]),
    'dbx_detect_scratch_bytes': (_I64, [_I32, _I32, _I32]),
    'dbx_detect': (C.c_int, [_VP, _VP, _VP, _VP, _I32, _I32, _I32, _D, _VP, _I32, _VP, _VP, _VP, _VP]),
    'dbx_detect_batch_scratch_bytes': (_I64, [_I32, _I32, _I32, _I32]),
    'dbx_detect_batch': (C.c_int, [_VP, _VP, _VP, _VP, _I32, _I32, _I32, _I32, _D, _VP, _I32, _VP, _VP, _VP, _VP]),
    'dbx_nms': (C.c_int, [_VP, _I32, _I32, _D, _VP, _VP, _VP]),
    'dbx_detect_thresh_batch_scratch_bytes': (_I64, [_I32, _I32, _I32, _I32]),
    'dbx_detect_thresh_batch': (C.c_int, [_VP, _VP, _VP, _VP, _I32, _I32, _I32, _F, _I32, _D, _VP, _I32, _VP, _VP, _VP, _VP, _VP]),
    'dbx_thresh_rows_batch_scratch_bytes': (_I64, [_I32, _I32, _I32, _I32]),
    'dbx_thresh_rows_batch': (C.c_int, [_VP, _VP, _VP, _VP, _I32, _I32, _I32, _F, _I32, _VP, _I32, _VP, _VP, _VP, _VP]),
    'dbx_nms_large_scratch_bytes': (_I64, [_I32]),
    'dbx_nms_large': (C.c_int, [_VP, _I32, _I32, _D, _VP, _VP, _VP]),
    'dbx_merge_nms_batch_workspace_bytes': (_I64, [_I32, _I32, _I32]),
    'dbx_merge_nms_batch': (C.c_int, [C.POINTER(C.c_void_p), C.POINTER(MergeXform), _I32, _I32, _I32, _I32, _D, _VP, _VP, _VP, _VP]),
    'dbx_merge_nms_thresh_batch_workspace_bytes': (_I64, [_I32, _I32, _I32]),
    'dbx_merge_nms_thresh_batch': (C.c_int, [C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(MergeXform), _I32, _I32, _I32, _I32, _D,
                                             _VP, _VP, _VP, _VP, _VP]),
    'dbx_tile_grid': (C.c_int, [_I32, _I32, _I32, _I32, _VP, _I32]),
    'dbx_tile_stage_bytes': (_I64, [_I32, _I32, _I32]),
    'dbx_tile_rows_batch': (C.c_int, [_VP, _VP, _VP, _VP, _I32, _I32, _I32, _I32, _I32, _I32, _VP, _VP]),
    'dbx_tile_nms_batch_workspace_bytes': (_I64, [_I32, _I32, _I32]),
    'dbx_tile_nms_batch': (C.c_int, [_VP, _VP, _I32, _I32, _I32, _I32, _D, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    'dbx_tile_host': (C.c_int, [_I32, _I64, _VP, _I32, _VP, _VP, _I32, _I32, _VP, _VP]),
}

ABI_VERSION = 13         # include/densebox_hip.h DBX_ABI_VERSION this binding was written against
_lib = None
MISSING = []


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError('libdensebox_hip.so is not built (%s). Run `python -c "import __graft_entry__ as g; '
                               'g.build()"`; densebox_amd has no fallback path.' % LIB_PATH)
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            try:
                fn = getattr(L, name)
            except AttributeError:         # header/library out of sync: tests/test_abi.py fails on any entry here
                MISSING.append(name)
                continue
            fn.restype = res
            fn.argtypes = args
        if 'dbx_version' not in MISSING and L.dbx_version() != ABI_VERSION:
            raise RuntimeError('libdensebox_hip.so at %s has ABI version %d, this binding needs %d (struct layouts / scratch '
                               'contracts differ): rebuild it' % (LIB_PATH, L.dbx_version(), ABI_VERSION))
        _lib = L
    return _lib


def check(rc):
    if rc != 0:
        raise RuntimeError('libdensebox_hip: %s (status %d)' % (lib().dbx_last_error().decode(), rc))


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def stream_ptr():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)
