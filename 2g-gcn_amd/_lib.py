"""ctypes binding of lib2ggcn_hip.so (C ABI declared in include/twog_gcn.h).

The product path has NO fallback: if the shared library is missing or an entry point is absent, importing/using the
kernels raises. Build it with ``python -c "import __graft_entry__ as g; g.build()"`` or ``make -C 2g-gcn_amd/csrc``.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# TWOG_LIB_PATH: another build of the same library (the diagnostic builds: make jitter, tools/stamps_probe.sh); never a fallback -- a path
# that does not load raises exactly like a missing default library
LIB_PATH = os.environ.get('TWOG_LIB_PATH') or os.path.join(_HERE, 'lib2ggcn_hip.so')

c_float_p = C.POINTER(C.c_float)
c_double_p = C.POINTER(C.c_double)
c_int64_p = C.POINTER(C.c_int64)


class Rows(C.Structure):  # twog_rows_t
    _fields_ = [('ptr', C.c_void_p), ('ld_outer', C.c_int64), ('ld_inner', C.c_int64), ('inner', C.c_int32),
                ('pad_', C.c_int32)]


class Gemm(C.Structure):  # twog_gemm_t
    _fields_ = [('A', Rows), ('B', Rows), ('C', Rows), ('bias', C.c_void_p), ('M', C.c_int32), ('N', C.c_int32),
                ('K', C.c_int32), ('act', C.c_int32), ('accumulate', C.c_int32), ('batch', C.c_int32),
                ('a_batch_stride', C.c_int64), ('b_batch_stride', C.c_int64), ('c_batch_stride', C.c_int64),
                ('a_colsum', C.c_void_p), ('a_colsum_accumulate', C.c_int32), ('pad2_', C.c_int32)]


GUARD_MAX = 16


class Guard(C.Structure):  # twog_guard_t
    _fields_ = [('words', C.c_void_p * GUARD_MAX), ('out', C.c_void_p * GUARD_MAX), ('n', C.c_int64 * GUARD_MAX),
                ('n_words', C.c_int32), ('n_out', C.c_int32)]


class GruStep(C.Structure):  # twog_gru_step_t
    _fields_ = [('gi', Rows), ('gi2', Rows), ('gh', Rows), ('h_prev', Rows), ('h_out', Rows), ('save', Rows),
                ('u', C.c_void_p), ('u_ld_outer', C.c_int64), ('u_ld_inner', C.c_int64), ('u_inner', C.c_int32),
                ('rows', C.c_int32), ('hidden', C.c_int32), ('pad_', C.c_int32)]


class GruStepBwd(C.Structure):  # twog_gru_step_bwd_t
    _fields_ = [('dh', Rows), ('dh2', Rows), ('save', Rows), ('h_prev', Rows), ('dgi', Rows), ('dgh', Rows),
                ('dh_prev', Rows), ('u', C.c_void_p), ('du', C.c_void_p), ('u_ld_outer', C.c_int64),
                ('u_ld_inner', C.c_int64), ('u_inner', C.c_int32), ('rows', C.c_int32), ('hidden', C.c_int32),
                ('dh_prev_accumulate', C.c_int32)]


class BiGru(C.Structure):  # twog_bigru_t
    _fields_ = [('gi', C.c_void_p), ('w_hh_f', C.c_void_p), ('b_hh_f', C.c_void_p), ('w_hh_r', C.c_void_p),
                ('b_hh_r', C.c_void_p), ('out', C.c_void_p), ('save', C.c_void_p), ('tmp_gh', C.c_void_p),
                ('zeros', C.c_void_p), ('E', C.c_int32), ('pad_', C.c_int32)]


class BiGruBwd(C.Structure):  # twog_bigru_bwd_t
    _fields_ = [('d_out', C.c_void_p), ('save', C.c_void_p), ('out', C.c_void_p), ('w_hh_f', C.c_void_p),
                ('w_hh_r', C.c_void_p), ('d_gi', C.c_void_p), ('d_gh', C.c_void_p), ('carry', C.c_void_p),
                ('E', C.c_int32), ('pad_', C.c_int32)]


class EntityPool(C.Structure):  # twog_entity_pool_t
    _fields_ = [('hfr', C.c_void_p), ('ofr', C.c_void_p), ('mask', C.c_void_p), ('hin', C.c_void_p), ('oin', C.c_void_p),
                ('bs', C.c_int32), ('T', C.c_int32), ('H', C.c_int32), ('O', C.c_int32), ('W', C.c_int32),
                ('pad_', C.c_int32)]


class EntityPoolBwd(C.Structure):  # twog_entity_pool_bwd_t
    _fields_ = [('d_hin', C.c_void_p), ('d_oin', C.c_void_p), ('mask', C.c_void_p), ('d_hfr', C.c_void_p),
                ('d_ofr', C.c_void_p), ('bs', C.c_int32), ('T', C.c_int32), ('H', C.c_int32), ('O', C.c_int32),
                ('W', C.c_int32), ('pad_', C.c_int32)]


class Attn(C.Structure):  # twog_attn_t
    _fields_ = [('feat_h', Rows), ('feat_o', Rows), ('msg_hh', Rows), ('msg_ho', Rows), ('msg_oh', Rows),
                ('msg_oo', Rows), ('msg_so', Rows), ('msg_sh', Rows), ('out_hh', Rows), ('out_oh', Rows),
                ('out_sh', Rows), ('out_ho', Rows), ('out_so', Rows), ('out_oo', Rows), ('obj_mask', C.c_void_p),
                ('att', C.c_void_p), ('n_inst', C.c_int32), ('inst_per_clip', C.c_int32), ('H', C.c_int32),
                ('O', C.c_int32), ('D', C.c_int32), ('hidden', C.c_int32), ('scale', C.c_float),
                ('recv_mask_ho', C.c_int32)]


class AttnBwd(C.Structure):  # twog_attn_bwd_t
    _fields_ = [('f', Attn), ('dout_hh', Rows), ('dout_oh', Rows), ('dout_sh', Rows), ('dout_ho', Rows),
                ('dout_so', Rows), ('dout_oo', Rows), ('dmsg_hh', Rows), ('dmsg_ho', Rows), ('dmsg_oh', Rows),
                ('dmsg_oo', Rows), ('dmsg_so', Rows), ('dmsg_sh', Rows), ('dfeat_h', Rows), ('dfeat_o', Rows),
                ('dw_extra', C.c_void_p), ('dfeat_accumulate', C.c_int32), ('relu_mask_dmsg', C.c_int32)]


class SegRnn(C.Structure):  # twog_segrnn_t
    _fields_ = [('bs', C.c_int32), ('T', C.c_int32), ('H', C.c_int32), ('O', C.c_int32), ('hidden', C.c_int32),
                ('msg_segment', C.c_int32), ('rel_hh', C.c_int32), ('rel_ho', C.c_int32), ('rel_oh', C.c_int32),
                ('rel_oo', C.c_int32), ('att_scale', C.c_float), ('pad_', C.c_int32),
                ('gi_h', C.c_void_p), ('gi_o', C.c_void_p), ('u_h', C.c_void_p), ('u_o', C.c_void_p),
                ('obj_mask', C.c_void_p),
                ('w_hh_h', C.c_void_p * 2), ('b_hh_h', C.c_void_p * 2), ('w_hh_o', C.c_void_p * 2),
                ('b_hh_o', C.c_void_p * 2), ('w_ihm_h', C.c_void_p * 2), ('w_ihm_o', C.c_void_p * 2),
                ('ld_ih_h', C.c_int64), ('ld_ih_o', C.c_int64),
                ('w_smsg_h', C.c_void_p), ('b_smsg_h', C.c_void_p), ('w_smsg_o', C.c_void_p), ('b_smsg_o', C.c_void_p),
                ('hs_h', C.c_void_p), ('hs_o', C.c_void_p), ('save_h', C.c_void_p), ('save_o', C.c_void_p),
                ('msrc_h', C.c_void_p), ('msrc_o', C.c_void_p), ('mg_h', C.c_void_p), ('mg_o', C.c_void_p),
                ('att', C.c_void_p), ('tmp_gim_h', C.c_void_p), ('tmp_gim_o', C.c_void_p), ('tmp_gh_h', C.c_void_p),
                ('tmp_gh_o', C.c_void_p), ('zeros', C.c_void_p)]


class SegRnnBwd(C.Structure):  # twog_segrnn_bwd_t
    _fields_ = [('d_hs_h', C.c_void_p), ('d_hs_o', C.c_void_p), ('d_gi_h', C.c_void_p), ('d_gi_o', C.c_void_p),
                ('d_gh_h', C.c_void_p), ('d_gh_o', C.c_void_p), ('d_u_h', C.c_void_p), ('d_u_o', C.c_void_p),
                ('d_pre_h', C.c_void_p), ('d_pre_o', C.c_void_p), ('carry_h', C.c_void_p), ('carry_o', C.c_void_p),
                ('tmp_dmg_h', C.c_void_p), ('tmp_dmg_o', C.c_void_p), ('trash', C.c_void_p), ('du_part_h', C.c_void_p),
                ('du_part_o', C.c_void_p)]


class Gate(C.Structure):  # twog_gate_t
    _fields_ = [('x', Rows), ('seg_col', C.c_int32 * 8), ('n_seg', C.c_int32), ('hidden', C.c_int32),
                ('w', C.c_void_p), ('b', C.c_void_p), ('noise', C.c_void_p), ('hard', C.c_void_p),
                ('soft', C.c_void_p), ('p_save', C.c_void_p), ('bs', C.c_int32), ('T', C.c_int32), ('E', C.c_int32),
                ('noise_entities', C.c_int32), ('noise_offset', C.c_int32), ('force_last', C.c_int32),
                ('threshold', C.c_float), ('pad_', C.c_int32)]


class Loss(C.Structure):  # twog_loss_t
    _fields_ = [('kind', C.c_int32), ('n_classes', C.c_int32), ('outer', C.c_int64), ('inner', C.c_int64),
                ('input', C.c_void_p), ('target', C.c_void_p), ('dinput', C.c_void_p), ('weight', C.c_float),
                ('ignore_value', C.c_float)]


class WLoss(C.Structure):  # twog_wloss_t
    _fields_ = Loss._fields_ + [('class_weight', C.c_void_p), ('positive_class_weight', C.c_float), ('pad0_', C.c_int32)]


class SmoothLoss(C.Structure):  # twog_smooth_loss_t
    _fields_ = [('n_classes', C.c_int32), ('pad0_', C.c_int32), ('outer', C.c_int64), ('steps', C.c_int64),
                ('entities', C.c_int64), ('input', C.c_void_p), ('target', C.c_void_p), ('dinput', C.c_void_p),
                ('weight', C.c_float), ('tau', C.c_float), ('ignore_value', C.c_float), ('accumulate', C.c_int32)]


class Relation(C.Structure):  # twog_relation_t
    _fields_ = [('q', Rows), ('k', Rows), ('msg', Rows), ('p_r', Rows), ('p_s', Rows), ('out', Rows),
                ('a_r', C.c_void_p), ('c_s', C.c_void_p), ('dist', C.c_void_p), ('dist_ld_inst', C.c_int64),
                ('dist_ld_r', C.c_int64), ('dist_ld_s', C.c_int64), ('send_mask', C.c_void_p),
                ('recv_mask', C.c_void_p), ('att', C.c_void_p), ('score_bias', C.c_void_p), ('scale', C.c_float),
                ('score_mode', C.c_int32), ('msg_mode', C.c_int32), ('relu_scores', C.c_int32),
                ('exclude_self', C.c_int32), ('n_inst', C.c_int32), ('inst_per_clip', C.c_int32), ('R', C.c_int32),
                ('S', C.c_int32), ('D', C.c_int32), ('hidden', C.c_int32), ('pad_', C.c_int32)]


class RowOp(C.Structure):  # twog_rowop_t
    _fields_ = [('a', Rows), ('b', Rows), ('dst', Rows), ('s', C.c_void_p), ('v', C.c_void_p), ('kind', C.c_int32),
                ('rows', C.c_int32), ('cols', C.c_int32), ('pad_', C.c_int32)]


class ColSum(C.Structure):  # twog_colsum_t
    _fields_ = [('x', Rows), ('rowscale', C.c_void_p), ('out', C.c_void_p), ('rows', C.c_int32), ('cols', C.c_int32),
                ('accumulate', C.c_int32), ('pad_', C.c_int32)]


COLSUM_MAX = 16   # TWOG_COLSUM_MAX


class Copy(C.Structure):  # twog_copy_t
    _fields_ = [('src', C.c_void_p), ('dst', C.c_void_p), ('n', C.c_int64)]


COPY_MAX = 16   # TWOG_COPY_MAX
PERSIST_NOT_RESIDENT = -3   # TWOG_PERSIST_NOT_RESIDENT

TAPE_GEMM, TAPE_RELATION_FWD, TAPE_RELATION_BWD, TAPE_GRU_STEP_FWD, TAPE_GRU_STEP_BWD, TAPE_ROWOPS = range(6)   # TWOG_TAPE_*


class TapeEntry(C.Structure):  # twog_tape_entry_t
    _fields_ = [('kind', C.c_int32), ('n', C.c_int32), ('flags', C.c_int32), ('pad_', C.c_int32), ('desc', C.c_void_p)]


class RelationBwd(C.Structure):  # twog_relation_bwd_t
    _fields_ = [('f', Relation), ('dout', Rows), ('dmsg', Rows), ('dp_r', Rows), ('dp_s', Rows), ('dq', Rows),
                ('dk', Rows), ('da_r', C.c_void_p), ('dc_s', C.c_void_p), ('dscore_sum', C.c_void_p),
                ('dq_accumulate', C.c_int32),
                ('dk_accumulate', C.c_int32), ('relu_mask_dmsg', C.c_int32), ('pad_', C.c_int32)]


REL_SUM, REL_DOT, REL_ADDITIVE, REL_DISTANCE, REL_MEAN = 0, 1, 2, 3, 4   # TWOG_REL_*
REL_MSG_SENDER, REL_MSG_PAIR = 0, 1

LOSS_MAX_TERMS, LOSS_BLOCKS = 16, 64  # TWOG_LOSS_MAX_TERMS, TWOG_LOSS_BLOCKS

NORM_MAX_RANGES, NORM_BLOCKS = 8, 2048   # TWOG_NORM_MAX_RANGES, TWOG_NORM_BLOCKS


class Ranges(C.Structure):  # twog_ranges_t
    _fields_ = [('begin', C.c_int64 * NORM_MAX_RANGES), ('end', C.c_int64 * NORM_MAX_RANGES), ('n_ranges', C.c_int32),
                ('pad_', C.c_int32)]


VITERBI_CHUNK = 16   # TWOG_VITERBI_CHUNK
VITERBI_ROUTES = ('lds', 'workspace')   # TWOG_VITERBI_ROUTE_LDS, TWOG_VITERBI_ROUTE_WORKSPACE


def viterbi_workspace(lib, bs, n_classes, T, E):
    """twog_viterbi_workspace of the loaded library `lib`: (route, bytes), route 'lds' or 'workspace'. No device is touched.
    ValueError beyond the limits of twog_viterbi_limits."""
    nbytes = C.c_size_t(0)
    rc = lib.twog_viterbi_workspace(int(bs), int(n_classes), int(T), int(E), C.byref(nbytes))
    if rc == -2:
        raise ValueError(f'the Viterbi decode takes up to 64 classes and 4096 model steps, not {n_classes} and {T}')
    if rc < 0:
        raise RuntimeError(f'twog_viterbi_workspace failed with code {rc}')
    return VITERBI_ROUTES[rc], nbytes.value


SEGDEC_MAX_DURATION = 128   # TWOG_SEGDEC_MAX_DURATION
SEGDEC_ROUTES = ('lds', 'workspace')   # TWOG_SEGDEC_ROUTE_LDS, TWOG_SEGDEC_ROUTE_WORKSPACE


def segdecode_plan(lib, bs, n_classes, T, E, D):
    """twog_segdecode_plan of the loaded library `lib` as a dict: class_template, waves (per workgroup), groups (workgroups
    per clip), route 'lds' or 'workspace', workspace_bytes. No device is touched. ValueError beyond the limits of
    twog_segdecode_limits."""
    out, nbytes = (C.c_int32 * 4)(), C.c_size_t(0)
    rc = lib.twog_segdecode_plan(int(bs), int(n_classes), int(T), int(E), int(D), out, C.byref(nbytes))
    if rc == -2:
        raise ValueError(f'the segmental decode takes up to 64 classes, 4096 model steps and durations up to '
                         f'{SEGDEC_MAX_DURATION}, not {n_classes}, {T} and {D}')
    if rc < 0:
        raise RuntimeError(f'twog_segdecode_plan failed with code {rc}')
    return {'class_template': out[0], 'waves': out[1], 'groups': out[2], 'route': SEGDEC_ROUTES[out[3]],
            'workspace_bytes': nbytes.value}


CRF_CHUNK, CRF_SEQ_WORDS = 16, 4   # TWOG_CRF_CHUNK, TWOG_CRF_SEQ_WORDS
SEMICRF_SEQ_WORDS = 4   # TWOG_SEMICRF_SEQ_WORDS


def crf_workspace(lib, bs, n_classes, T, E):
    """twog_crf_workspace of the loaded library `lib`: the bytes of (alpha, seq, partials). No device is touched.
    ValueError beyond the limits of twog_crf_limits."""
    alpha, seq, partials = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0)
    rc = lib.twog_crf_workspace(int(bs), int(n_classes), int(T), int(E), C.byref(alpha), C.byref(seq), C.byref(partials))
    if rc == -2:
        raise ValueError(f'the CRF loss takes up to 64 classes and 4096 model steps, not {n_classes} and {T}')
    if rc < 0:
        raise RuntimeError(f'twog_crf_workspace failed with code {rc}')
    return alpha.value, seq.value, partials.value


def semicrf_plan(lib, bs, n_classes, T, E, D):
    """twog_semicrf_plan of the loaded library `lib` as a dict: class_template, fwd_waves / fwd_groups and bwd_waves /
    bwd_groups (waves per workgroup, workgroups per clip), and the bytes of the workspaces ed_bytes, marks_bytes, seq_bytes,
    partial_bytes. No device is touched. ValueError beyond the limits of twog_semicrf_limits."""
    out, nbytes = (C.c_int32 * 5)(), (C.c_size_t * 4)()
    rc = lib.twog_semicrf_plan(int(bs), int(n_classes), int(T), int(E), int(D), out, nbytes)
    if rc == -2:
        raise ValueError(f'the semi-Markov CRF loss takes up to 64 classes, 4096 model steps and durations up to '
                         f'{SEGDEC_MAX_DURATION}, not {n_classes}, {T} and {D}')
    if rc < 0:
        raise RuntimeError(f'twog_semicrf_plan failed with code {rc}')
    return {'class_template': out[0], 'fwd_waves': out[1], 'fwd_groups': out[2], 'bwd_waves': out[3], 'bwd_groups': out[4],
            'ed_bytes': nbytes[0], 'marks_bytes': nbytes[1], 'seq_bytes': nbytes[2], 'partial_bytes': nbytes[3]}


BIGRU_PLAN_HEAD, BIGRU_PLAN_MAX_COMBOS = 8, 32   # TWOG_BIGRU_PLAN_HEAD, TWOG_BIGRU_PLAN_MAX_COMBOS
BIGRU_PLAN_INTS = BIGRU_PLAN_HEAD + 4 * BIGRU_PLAN_MAX_COMBOS   # TWOG_BIGRU_PLAN_INTS


def bigru_persistent_plan(lib, Es, bs, h, n_cus=0):
    """twog_bigru_persistent_plan of the loaded library `lib` as a dict (include/twog_gcn.h states every field); with n_cus > 0
    no device is touched. served False: the shape is refused, the other fields but n_cus are 0 / empty."""
    out = (C.c_int32 * BIGRU_PLAN_INTS)()
    rc = lib.twog_bigru_persistent_plan((C.c_int32 * max(1, len(Es)))(*Es), len(Es), bs, h, n_cus, out)
    if rc != 0:
        raise RuntimeError(f'twog_bigru_persistent_plan failed with code {rc}')
    n = max(0, out[0])
    combos = [tuple(out[BIGRU_PLAN_HEAD + 4 * i:BIGRU_PLAN_HEAD + 4 * i + 4]) for i in range(n)]
    return dict(served=out[0] > 0, n_combos=out[0], nkb=out[1], twc=out[2], grid=out[3], lds_fwd=out[4], lds_bwd=out[5],
                bwd_served=bool(out[6]), n_cus=out[7], combos=combos)


SEGRNN_PLAN_INTS = 16   # TWOG_SEGRNN_PLAN_INTS
SEGRNN_PLAN_FIELDS = ('served', 'cpc', 'n_chunks', 'last', 'mh', 'mo', 'pair_mask', 'grid', 'lds_fwd', 'lds_bwd', 'x3q1', 'dw_pad',
                      'sync_words')   # out[0 .. 12]


def segrnn_persistent_plan(lib, bs, T, H, O, h, n_cus=0, msg_segment=True, rels=(True, True, True, True)):
    """twog_segrnn_persistent_plan of the loaded library `lib` as a dict (include/twog_gcn.h states every field); with n_cus > 0
    no device is touched. A shape query: the descriptor carries no buffer. served False: the shape is refused, the other fields
    but n_cus are 0."""
    s = SegRnn()
    s.bs, s.T, s.H, s.O, s.hidden, s.msg_segment = int(bs), int(T), int(H), int(O), int(h), int(bool(msg_segment))
    s.rel_hh, s.rel_ho, s.rel_oh, s.rel_oo = (int(bool(r)) for r in rels)
    out = (C.c_int32 * SEGRNN_PLAN_INTS)()
    rc = lib.twog_segrnn_persistent_plan(C.byref(s), int(n_cus), out)
    if rc != 0:
        raise RuntimeError(f'twog_segrnn_persistent_plan failed with code {rc}')
    p = dict(zip(SEGRNN_PLAN_FIELDS, out[:13]))
    p.update(served=bool(out[0]), x3q1=bool(out[10]), pair_mask=out[6] & 0xffffffff, scratch_bytes=out[13] + (out[14] << 31),
             n_cus=out[15])
    return p


MTL_PASS, MTL_SOFTMAX, MTL_MSE, MTL_MAE = 0, 1, 2, 3   # TWOG_MTL_*
MTL_MAX_TERMS = 16   # TWOG_MTL_MAX_TERMS


class Mtl(C.Structure):  # twog_mtl_t
    _fields_ = [('kind', C.c_int32 * MTL_MAX_TERMS), ('n', C.c_int32), ('pad_', C.c_int32)]


OPTIM_CLIP, OPTIM_DECOUPLED, OPTIM_SKIP_NONFINITE = 1, 2, 4   # TWOG_OPTIM_*


class OptimState(C.Structure):  # twog_optim_state_t: the 64-byte step state of the device-side Adam
    _fields_ = [('step', C.c_int64), ('skipped', C.c_int64), ('beta1_pow', C.c_double), ('beta2_pow', C.c_double),
                ('lr', C.c_float), ('step_size', C.c_float), ('bc2s', C.c_float), ('clip_k', C.c_float),
                ('decay_mul', C.c_float), ('apply', C.c_int32), ('reserved_', C.c_int64)]


class OptimHyper(C.Structure):  # twog_optim_hyper_t
    _fields_ = [('beta1', C.c_float), ('beta2', C.c_float), ('eps', C.c_float), ('weight_decay', C.c_float),
                ('grad_scale', C.c_float), ('ema_decay', C.c_float)]

AUGMENT_TAG_GEOMETRY, AUGMENT_TAG_HUMAN, AUGMENT_TAG_OBJECT = 0x47454F4D, 0x48554D4E, 0x4F424A53   # TWOG_AUGMENT_TAG_*


class Augment(C.Structure):  # twog_augment_t
    _fields_ = [('x_human', C.c_void_p), ('x_objects', C.c_void_p), ('clip_ids', C.c_void_p), ('steps', C.c_void_p),
                ('objects_mask', C.c_void_p), ('state', C.c_void_p), ('params_out', C.c_void_p),
                ('bs', C.c_int32), ('T', C.c_int32), ('H', C.c_int32), ('O', C.c_int32), ('F_h', C.c_int32),
                ('F_o', C.c_int32), ('N', C.c_int32), ('geo_offset', C.c_int32),
                ('tan_half_max', C.c_float), ('scale_max', C.c_float), ('shift_max', C.c_float), ('cx', C.c_float),
                ('cy', C.c_float), ('amp', C.c_float), ('keep_scale', C.c_float), ('drop_threshold', C.c_uint32)]


# name -> (argtypes) ; every function returns int except twog_version
_I, _L, _F, _P = C.c_int, C.c_int64, C.c_float, C.c_void_p
SIGNATURES = {
    'twog_gemm_f32': [C.POINTER(Gemm), _I, _I, _I, _P, C.c_size_t, _P],
    'twog_guard_outputs': [C.POINTER(Guard), _P],
    'twog_stream_create_masked': [_I, C.POINTER(C.c_void_p)],
    'twog_stream_create_low_priority': [C.POINTER(C.c_void_p)],
    'twog_stream_destroy': [_P],
    'twog_gemm_colsum_fused': [C.POINTER(Gemm), _I, _I, _I, _P, C.c_size_t],
    'twog_gemm_last_class': [],
    'twog_gemm_set_precision': [_I],
    'twog_gemm_get_precision': [],
    'twog_chain_workspace_bytes': [],
    'twog_gemm_f32_chain': [C.POINTER(Gemm), _I, _I, _I, _P, C.c_size_t, _P],
    'twog_gcn_max_nodes': [],
    'twog_gcn_launch_plan': [_I, _I, _I, C.POINTER(C.c_int)],
    'twog_bn_stats': [_P, _L, _I, _I, _P, _I, _P],
    'twog_bn_finalize': [_P, _I, _I, _I, _P, _P, _P, _P, _P, _I, _P, _P, _P, _P, _P, _P, _P],
    'twog_gcn_embed1_fwd': [_P, _L, _I, _I, _P, _P, _P, _P, _P],
    'twog_gcn_fused_fwd': [_P, _L, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P],
    'twog_gcn_embed1_bwd': [_P, _L, _I, _I, _P, _P, _P, _P, _P, _I, _P, _P, _P, _P, _P],
    'twog_gcn_input_bwd': [_P, _L, _I, _I, _I, _L, _P, _P, _P, _P, _P, _P, _I, _P, _I, _P],
    'twog_gcn_attn_fwd': [_P, _P, _I, _I, _P, _P, _P],
    'twog_gcn_attn_bwd': [_P, _P, _P, _P, _I, _I, _P, _P, _P],
    'twog_gcn_attn2_fwd': [_P, _P, _I, _I, _P, _P, _P],
    'twog_gcn_attn2_bwd_blocks': [_I],
    'twog_gcn_attn2_bwd': [_P, _P, _P, _P, _I, _I, _P, _P, _I, _P],
    'twog_gcn_wide_max_nodes': [],
    'twog_gcn_wide_launch_plan': [_I, _I, _I, C.POINTER(C.c_int)],
    'twog_gcn_wide_bn_stats': [_P, _L, _I, _I, _P, _I, _P],
    'twog_gcn_wide_bn_finalize': [_P, _I, _I, _I, _P, _P, _P, _P, _P, _I, _P, _P, _P, _P, _P, _P, _P],
    'twog_gcn_wide_embed1_fwd': [_P, _L, _I, _I, _P, _P, _P, _P, _P],
    'twog_gcn_wide_embed1_bwd': [_P, _L, _I, _I, _P, _P, _P, _P, _P, _I, _P, _P, _P, _P, _P],
    'twog_gcn_wide_input_bwd': [_P, _L, _I, _I, _I, _L, _P, _P, _P, _P, _P, _P, _I, _P, _I, _P],
    'twog_gcn_wide_fwd': [_P, _L, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P],
    'twog_gcn_wide_bwd': [_P, _P, _P, _P, _I, _I, _P, _P, _I, _P],
    'twog_gru_step_fwd': [C.POINTER(GruStep), _I, _P],
    'twog_gru_step_bwd': [C.POINTER(GruStepBwd), _I, _P],
    'twog_gru_step_last_path': [],
    'twog_bigru_fwd': [C.POINTER(BiGru), _I, _I, _I, _I, _P, C.c_size_t, _P],
    'twog_bigru_persistent_supported': [C.POINTER(BiGru), _I, _I, _I],
    'twog_bigru_fwd_persistent': [C.POINTER(BiGru), _I, _I, _I, _I, _P, _P],
    'twog_bigru_bwd_persistent_supported': [C.POINTER(BiGruBwd), _I, _I, _I],
    'twog_bigru_bwd_persistent': [C.POINTER(BiGruBwd), _I, _I, _I, _I, _P, _P],
    'twog_bigru_persistent_plan': [C.POINTER(C.c_int32), _I, _I, _I, _I, C.POINTER(C.c_int32)],
    'twog_bigru_bwd': [C.POINTER(BiGruBwd), _I, _I, _I, _I, _P, C.c_size_t, _P],
    'twog_gru_seq_fwd': [C.POINTER(BiGru), _I, _I, _I, _I, _P, C.c_size_t, _P],
    'twog_gru_seq_bwd': [C.POINTER(BiGruBwd), _I, _I, _I, _I, _P, C.c_size_t, _P],
    'twog_entity_pool_fwd': [C.POINTER(EntityPool), _P],
    'twog_entity_pool_bwd': [C.POINTER(EntityPoolBwd), _P],
    'twog_attn_fwd': [C.POINTER(Attn), _I, _P],
    'twog_attn_limits': [C.POINTER(C.c_int), C.POINTER(C.c_int)],
    'twog_attn_bwd': [C.POINTER(AttnBwd), _I, _P],
    'twog_attn_last_path': [],
    'twog_segrnn_fwd': [C.POINTER(SegRnn), _P, C.c_size_t, _P],
    'twog_segrnn_bwd': [C.POINTER(SegRnn), C.POINTER(SegRnnBwd), _P, C.c_size_t, _P],
    'twog_segrnn_persistent_supported': [C.POINTER(SegRnn)],
    'twog_segrnn_persistent_sync_bytes': [],
    'twog_segrnn_fwd_persistent': [C.POINTER(SegRnn), _P, _P],
    'twog_segrnn_bwd_persistent_scratch_bytes': [C.POINTER(SegRnn)],
    'twog_segrnn_bwd_persistent': [C.POINTER(SegRnn), C.POINTER(SegRnnBwd), _P, C.c_size_t, _P, _P],
    'twog_segrnn_persistent_plan': [C.POINTER(SegRnn), _I, C.POINTER(C.c_int32)],
    'twog_graph_cache_stats': [c_int64_p, c_int64_p],
    'twog_pos_embed_fwd': [_P, _P, _I, _I, _I, _I, _P, _P, _I, _I, Rows, _P, _P],
    'twog_periodic_embed_bwd': [Rows, _P, _I, _I, _P, _P],
    'twog_seglen_fwd': [_P, _P, _I, _I, _I, _I, _P, _P],
    'twog_seglen_bwd': [_P, _P, _I, _I, _I, _I, _P, _P, _P],
    'twog_mul': [_P, _P, _P, _L, _I, _P],
    'twog_scale_rows': [Rows, _P, _I, _I, _P],
    'twog_relation_limits': [],
    'twog_relation_fwd': [C.POINTER(Relation), _P],
    'twog_relation_bwd': [C.POINTER(RelationBwd), _P],
    'twog_relation_fwd_n': [C.POINTER(Relation), _I, _P],
    'twog_relation_bwd_n': [C.POINTER(RelationBwd), _I, _P],
    'twog_ssp_fwd': [_P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P],
    'twog_ssp_gather': [_P, _L, _P, _L, _L, _I, _P, _I, _I, _I, _I, _I, _P],
    'twog_ssp_bwd': [_P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P],
    'twog_gate_fwd': [C.POINTER(Gate), _P],
    'twog_gate_bwd': [C.POINTER(Gate), _P, _P, _P, _P, _P],
    'twog_gumbel_noise_fill': [_P, _I, _I, _I, C.c_uint32, _P, _P, _P],
    'twog_augment_inputs': [C.POINTER(Augment), _P],
    'twog_augment_grid': [_L],
    'twog_rank1_update': [Rows, _P, _P, _I, _I, _P],
    'twog_colsum': [Rows, _P, _I, _I, _P, _I, _P, _I, _P],
    'twog_colsum_n_partial_floats': [C.POINTER(ColSum), _I],
    'twog_colsum_n': [C.POINTER(ColSum), _I, _P, C.c_size_t, _P],
    'twog_filter_fwd': [_P, _P, _P, _I, _I, _I, _F, _P],
    'twog_reorder_fwd': [_P, _P, _P, _I, _I, _I, _I, _P],
    'twog_reorder_bwd': [_P, _P, _P, _I, _I, _I, _I, _P],
    'twog_logsoftmax_permute_fwd': [_P, _P, _I, _I, _I, _I, _P],
    'twog_logsoftmax_permute_bwd': [_P, _P, _P, _I, _I, _I, _I, _P],
    'twog_relu_bwd': [Rows, Rows, Rows, _I, _I, _P],
    'twog_add_rows': [Rows, Rows, _I, _I, _P],
    'twog_rowops': [C.POINTER(RowOp), _I, _P],
    'twog_tape_run': [C.POINTER(TapeEntry), C.POINTER(TapeEntry), _I, _I, _I, _P, C.c_size_t, _P],
    'twog_fill_zero': [_P, C.c_size_t, _P],
    'twog_copy_blocks': [C.POINTER(Copy), _I, _P],
    'twog_debug_occupy': [_I, _I, _I, _P],
    'twog_adam_step': [_P, _P, _P, _P, _L, _F, _F, _F, _F, _F, _I, _F, _P],
    'twog_stream_grid': [_I, _L, _L],
    'twog_multitask_loss_fwd': [C.POINTER(Loss), _I, _P, _P, _P, _P],
    'twog_multitask_loss_bwd': [C.POINTER(Loss), _I, _P, _P, _P],
    'twog_smooth_loss_fwd': [C.POINTER(SmoothLoss), _I, _P, _P, _P, _P],
    'twog_smooth_loss_bwd': [C.POINTER(SmoothLoss), _I, _P, _P, _P],
    'twog_weighted_loss_fwd': [C.POINTER(WLoss), _I, _P, _P, _P, _P],
    'twog_weighted_loss_bwd': [C.POINTER(WLoss), _I, _P, _P, _P],
    'twog_grad_norm': [_P, C.POINTER(Ranges), _F, _F, _P, _P, _P],
    'twog_adam_step_coef': [_P, _P, _P, _P, _L, _F, _F, _F, _F, _F, _I, _F, _P, _P],
    'twog_mtl_weight_fwd': [C.POINTER(Mtl), _P, _P, _P, _P],
    'twog_mtl_weight_bwd': [C.POINTER(Mtl), _P, _P, _P, _P, _P, _I, _P],
    'twog_optim_prepare': [_P, C.POINTER(OptimHyper), _F, _P, C.POINTER(C.c_void_p), _I, _P, _I, _P],
    'twog_optim_apply': [_P, _P, _P, _P, _P, _L, C.POINTER(OptimHyper), _I, _P, _P],
    'twog_predict_labels': [_P, _I, _I, _I, _I, _I, _I, _P, _P],
    'twog_f1_at_k': [_P, _P, _I, _I, _I, C.c_double, _L, _I, _P, _P, _P, _P],
    'twog_eval_update': [_P, _I, _I, _I, _I, _I, _P, _I, _P, _I, _P, _P, _P, _P, _P],
    'twog_confusion_counts': [_P, _P, _L, _I, _P, _P, _P],
    'twog_class_counts': [_P, _L, _I, _L, _P, _P],
    'twog_eval_limits': [C.POINTER(C.c_int), C.POINTER(C.c_int)],
    'twog_segment_f1': [_P, _P, _I, _I, _I, _I, C.POINTER(C.c_double), _I, _L, _I, _P, _P, _P, _P, _P, _P],
    'twog_segment_f1_accumulate': [_P, _P, _I, _I, _P, _P, _P],
    'twog_segment_f1_limits': [C.POINTER(C.c_int), C.POINTER(C.c_int)],
    'twog_segment_edit': [_P, _P, _I, _I, _I, _L, _I, _L, _I, _P, _P, _P, _P, _P, _P],
    'twog_segment_edit_limits': [C.POINTER(C.c_int)],
    'twog_viterbi_limits': [C.POINTER(C.c_int), C.POINTER(C.c_int)],
    'twog_viterbi_workspace': [_I, _I, _I, _I, C.POINTER(C.c_size_t)],
    'twog_viterbi_decode': [_P, _I, _I, _I, _I, _P, _P, _P, _I, _I, _P, _P, _P, C.c_size_t, _P],
    'twog_transition_counts': [_P, _I, _I, _I, _I, _I, _L, _P, _P],
    'twog_segdecode_limits': [C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)],
    'twog_segdecode_plan': [_I, _I, _I, _I, _I, C.POINTER(C.c_int32), C.POINTER(C.c_size_t)],
    'twog_segdecode': [_P, _I, _I, _I, _I, _P, _P, _P, _I, _P, _I, _I, _P, _P, _P, C.c_size_t, _P],
    'twog_duration_counts': [_P, _I, _I, _I, _I, _I, _I, _L, _P, _P],
    'twog_crf_limits': [C.POINTER(C.c_int), C.POINTER(C.c_int)],
    'twog_crf_workspace': [_I, _I, _I, _I, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)],
    'twog_crf_nll_fwd': [_P, _P, _I, _I, _I, _I, _P, _P, _L, _F, _P, _P, _P, _P, _P],
    'twog_crf_nll_bwd': [_P, _P, _I, _I, _I, _I, _P, _L, _F, _P, _P, _P, _P, _P, _I, _P, _P, _P, _I, _P],
    'twog_semicrf_limits': [C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)],
    'twog_semicrf_plan': [_I, _I, _I, _I, _I, C.POINTER(C.c_int32), C.POINTER(C.c_size_t)],
    'twog_semicrf_nll_fwd': [_P, _P, _I, _I, _I, _I, _P, _P, _P, _I, _L, _F, _P, _P, _P, _P, _P, _P],
    'twog_semicrf_nll_bwd': [_P, _P, _I, _I, _I, _I, _P, _P, _I, _L, _F, _P, _P, _P, _P, _P, _P, _I, _P, _P, _P, _P, _I, _P],
}

_lib = None


def load():
    """Load lib2ggcn_hip.so and bind every entry point of include/twog_gcn.h. Raises if anything is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f'{LIB_PATH} not found: the HIP kernels are not built (run __graft_entry__.build() or '
                           f'`make -C 2g-gcn_amd/csrc`). There is no fallback path.')
    lib = C.CDLL(LIB_PATH)
    for name, argtypes in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is missing
        fn.argtypes = argtypes
        fn.restype = C.c_int
    lib.twog_chain_workspace_bytes.restype = C.c_size_t
    lib.twog_colsum_n_partial_floats.restype = C.c_size_t
    lib.twog_segrnn_persistent_sync_bytes.restype = C.c_size_t
    lib.twog_segrnn_bwd_persistent_scratch_bytes.restype = C.c_size_t
    lib.twog_version.restype = C.c_char_p
    lib.twog_version.argtypes = []
    _lib = lib
    return lib


def exported_symbols():
    return ['twog_version'] + list(SIGNATURES.keys())
