"""Python mirror of the jmh_* C ABI (include/jmhip.h) — the MI355X JM hot path.

This module is the host-side interface tests and bench.py drive: it mirrors lencod's per-picture
use of the hot path (JM 8.6 image.c › encode_one_frame → encode_one_macroblock per MB [J]) over
ctypes.  It loads ``csrc/libjmhip.so`` (built in-tree) and fails loudly if it is missing: there is
no CPU fallback in the product path.  ``libjmhost.so`` (host plumbing: synthetic source, CAVLC
writer, deblocking) is loaded on demand for the synthetic input generator.
"""
import ctypes
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("JMH_LIB_PATH") or os.path.join(HERE, "csrc", "libjmhip.so")   # override: A/B builds
HOST_LIB_PATH = os.path.join(HERE, "host", "build", "libjmhost.so")

JMH_OK = 0
JMH_E_INVALID_ARG, JMH_E_HIP, JMH_E_OOM, JMH_E_UNSUPPORTED_CFG, JMH_E_STATE, JMH_E_NO_DEVICE = -1, -2, -3, -4, -5, -6
JMH_P_SLICE, JMH_I_SLICE = 0, 2
JMH_ABI_VERSION = 14
JMH_FLAG_KERNEL_TIMING = 1
STATUS = {0: "ok", -1: "invalid argument", -2: "HIP runtime error", -3: "out of memory",
          -4: "unsupported configuration", -5: "invalid call order", -6: "no HIP device"}
# JM 8.6 rdopt.c QP2QUANT [J]: RDO-off lambda = QP2QUANT[max(0, qp-12)]
QP2QUANT = [1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 4, 4, 4, 5, 6, 6, 7, 8, 9, 10, 11, 13, 14, 16, 18,
            20, 23, 25, 29, 32, 36, 40, 45, 51, 57, 64, 72, 81, 91]


def lambda_rdo_off(qp):
    return QP2QUANT[max(0, qp - 12)]


def lambda_rdo_on(qp, bit_depth=8):
    """RDOptimization 1 (host/encoder.c jm_lambda_rdo_on): (lambda_mode, LAMBDA_FACTOR(sqrt(lambda_mode)))
    with lambda_mode = 0.85 * 2^((qp + QpBdOffsetY - 12) / 3) -- the same libm pow / sqrt as the C host."""
    import math
    qpbd = 6 * (bit_depth - 8) if bit_depth > 8 else 0
    lam = 0.85 * math.pow(2.0, (qp + qpbd - 12) / 3.0)
    return lam, int(65536.0 * math.sqrt(lam) + 0.5)


class JmhConfig(ctypes.Structure):
    _fields_ = [("width", ctypes.c_int32), ("height", ctypes.c_int32),
                ("search_range", ctypes.c_int32), ("search_mode", ctypes.c_int32),
                ("use_hadamard", ctypes.c_int32), ("restrict_search_range", ctypes.c_int32),
                ("inter_search", ctypes.c_int32 * 8), ("num_ref_frames", ctypes.c_int32),
                ("constrained_intra_pred", ctypes.c_int32), ("num_frame_slots", ctypes.c_int32),
                ("flags", ctypes.c_int32), ("pipeline_depth", ctypes.c_int32),
                ("transform_8x8_mode", ctypes.c_int32), ("jm_version", ctypes.c_int32),
                ("quant_offset", ctypes.c_int32 * 2), ("epzs_dual_refinement", ctypes.c_int32),
                ("slice_mbs", ctypes.c_int32), ("bit_depth", ctypes.c_int32),
                ("rdo", ctypes.c_int32), ("symbol_mode", ctypes.c_int32),
                ("epzs_subpel_me", ctypes.c_int32), ("epzs_subpel_thres_scale", ctypes.c_int32),
                ("epzs_min_thres_scale", ctypes.c_int32), ("epzs_max_thres_scale", ctypes.c_int32)]


class JmhFrameParams(ctypes.Structure):
    _fields_ = [("slice_type", ctypes.c_int32), ("qp", ctypes.c_int32),
                ("lambda_mode", ctypes.c_int32), ("lambda_motion", ctypes.c_int32),
                ("chroma_qp_offset", ctypes.c_int32), ("deblock", ctypes.c_int32),
                ("lf_disable", ctypes.c_int32), ("lf_alpha_div2", ctypes.c_int32),
                ("lf_beta_div2", ctypes.c_int32), ("lambda_factor_rd", ctypes.c_int32),
                ("lambda_rd", ctypes.c_double)]


class JmhTiming(ctypes.Structure):
    _fields_ = [("interp_ms", ctypes.c_float), ("mb_ms", ctypes.c_float),
                ("total_ms", ctypes.c_float), ("mb_launches", ctypes.c_int32),
                ("pictures", ctypes.c_int32), ("interps", ctypes.c_int32),
                ("analyse_ms", ctypes.c_float), ("analyse_launches", ctypes.c_int32),
                ("final_ms", ctypes.c_float), ("final_launches", ctypes.c_int32),
                ("ticks", ctypes.c_int32), ("tick_mbs", ctypes.c_int32),
                ("pictures_done", ctypes.c_int32),
                ("flow_launches", ctypes.c_int32), ("flow_mbs", ctypes.c_int32)]


class JmhBlockSearch(ctypes.Structure):
    _fields_ = [("mb_x", ctypes.c_int32), ("mb_y", ctypes.c_int32), ("blocktype", ctypes.c_int32),
                ("block_x", ctypes.c_int32), ("block_y", ctypes.c_int32), ("pred_mv", ctypes.c_int32 * 2),
                ("centre", ctypes.c_int32 * 2), ("search_range", ctypes.c_int32), ("lambda_factor", ctypes.c_int32),
                ("search_mode", ctypes.c_int32), ("slice_p", ctypes.c_int32)]


class JmhBlockResult(ctypes.Structure):
    _fields_ = [("mv", ctypes.c_int32 * 2), ("min_mcost", ctypes.c_int32), ("fullpel_mv", ctypes.c_int32 * 2),
                ("fullpel_cost", ctypes.c_int32)]


# jmh_mb_result, field for field (include/jmhip.h)
MB_RESULT_DTYPE = np.dtype([
    ("mb_type", "<i2"), ("cbp", "<i2"), ("cbp_blk", "<i4"), ("b8mode", "i1", 4),
    ("ref_idx", "i1", 4), ("i16mode", "i1"), ("c_ipred_mode", "i1"), ("transform_8x8", "i1"), ("pad0", "i1"),
    ("ipred", "i1", 16), ("mv", "<i2", (16, 2)), ("luma", "<i2", (16, 16)),
    ("luma_dc", "<i2", 16), ("chroma_dc", "<i2", (2, 4)), ("chroma_ac", "<i2", (2, 4, 16)),
    ("min_cost", "<i4"), ("reserved", "<i4")])

_P = ctypes.c_void_p
_I = ctypes.c_int
_SIGS = {
    "jmh_create": (_I, [ctypes.POINTER(JmhConfig), _I, ctypes.POINTER(_P)]),
    "jmh_destroy": (None, [_P]),
    "jmh_strerror": (ctypes.c_char_p, [_I]),
    "jmh_abi_version": (_I, []),
    "jmh_device_count": (_I, []),
    "jmh_set_reference": (_I, [_P, _I, _I, _P, _P, _P, _I, _I]),
    "jmh_frame_submit": (_I, [_P, _P, _P, _P, _I, _I, ctypes.POINTER(JmhFrameParams)]),
    "jmh_frame_wait": (_I, [_P]),
    "jmh_frame_push": (_I, [_P, _P, _P, _P, _I, _I, ctypes.POINTER(JmhFrameParams)]),
    "jmh_frame_pop": (_I, [_P]),
    "jmh_pipeline_depth": (_I, [_P]),
    "jmh_get_mb_result": (_P, [_P, _I]),
    "jmh_read_recon": (_I, [_P, _P, _P, _P, _I, _I]),
    "jmh_read_deblocked": (_I, [_P, _P, _P, _P, _I, _I]),
    "jmh_load_frame": (_I, [_P, _I, _P, _P, _P, _I, _I]),
    "jmh_set_reference_slot": (_I, [_P, _I]),
    "jmh_encode_slot": (_I, [_P, _I, ctypes.POINTER(JmhFrameParams)]),
    "jmh_sync": (_I, [_P]),
    "jmh_wait_issued": (_I, [_P]),
    "jmh_get_timing": (_I, [_P, ctypes.POINTER(JmhTiming)]),
    "jmh_ffs_sad_table": (_I, [_P, _I, _P, _P, _P]),
    "jmh_tq4x4_batch": (_I, [_P, _I, _P, _P, _I, _I, _P, _P, _P, _P]),
    "jmh_tq8x8_batch": (_I, [_P, _I, _P, _P, _I, _I, _P, _P, _P, _P]),
    "jmh_read_qpel": (_I, [_P, _P]),
    "jmh_set_reference_u16": (_I, [_P, _I, _I, _P, _P, _P, _I, _I]),
    "jmh_frame_submit_u16": (_I, [_P, _P, _P, _P, _I, _I, ctypes.POINTER(JmhFrameParams)]),
    "jmh_frame_push_u16": (_I, [_P, _P, _P, _P, _I, _I, ctypes.POINTER(JmhFrameParams)]),
    "jmh_read_recon_u16": (_I, [_P, _P, _P, _P, _I, _I]),
    "jmh_read_deblocked_u16": (_I, [_P, _P, _P, _P, _I, _I]),
    "jmh_load_frame_u16": (_I, [_P, _I, _P, _P, _P, _I, _I]),
    "jmh_search_pictures": (_I, [_P, _P, _P, _I]),
    "jmh_block_motion_search": (_I, [_P, _I, _P, _P]),
    "jmh_search_pictures_u16": (_I, [_P, _P, _P, _I, _I]),
    "jmh_block_motion_search_u16": (_I, [_P, _I, _P, _P]),
    "jmh_ffs_sad_table_u16": (_I, [_P, _I, _P, _P, _P]),
    "jmh_tq4x4_batch_u16": (_I, [_P, _I, _P, _P, _I, _I, _I, _P, _P, _P, _P]),
    "jmh_tq8x8_batch_u16": (_I, [_P, _I, _P, _P, _I, _I, _I, _P, _P, _P, _P]),
}
EXPORTED = tuple(_SIGS)


# ---- CAVLC slice data on the device (include/jmhip_cavlc.h; additive to ABI 14) ----
class JmhSliceDesc(ctypes.Structure):
    _fields_ = [("first_mb", ctypes.c_int32), ("n_mb", ctypes.c_int32), ("slice_type", ctypes.c_int32),
                ("lead_nbits", ctypes.c_int32), ("lead_bits", ctypes.c_uint32)]


class JmhSliceBytes(ctypes.Structure):
    _fields_ = [("offset", ctypes.c_int64), ("nbytes", ctypes.c_int64), ("nbits", ctypes.c_int64)]


JMW_MB_MAX_BITS = 15424          # csrc/jmh_cavlc_write.h: the worst case of one macroblock
_SIGS_CAVLC = {
    "jmh_cavlc_write_slices": (_I, [_P, _I, _P, _P, ctypes.c_size_t, _P]),
    "jmh_cavlc_write_results": (_I, [_P, _P, _I, _P, _P, ctypes.c_size_t, _P]),
}
EXPORTED_CAVLC = tuple(_SIGS_CAVLC)


def slice_descs(nmb, slice_type, mbs_per_slice=0, lead=()):
    """Raster runs of mbs_per_slice macroblocks (0: one slice) covering nmb macroblocks, as a
    JmhSliceDesc array; lead: (lead_nbits, lead_bits) per slice, cycled (default: none)."""
    step = mbs_per_slice if mbs_per_slice > 0 else nmb
    firsts = list(range(0, nmb, step))
    d = (JmhSliceDesc * len(firsts))()
    for i, f in enumerate(firsts):
        nb, bits = lead[i % len(lead)] if lead else (0, 0)
        d[i] = JmhSliceDesc(f, min(step, nmb - f), slice_type, nb, bits & ((1 << nb) - 1))
    return d


# ---- CABAC slice data on the device (include/jmhip_cabac.h; additive to ABI 14) ----
class JmhCabacSliceDesc(ctypes.Structure):
    _fields_ = [("first_mb", ctypes.c_int32), ("n_mb", ctypes.c_int32), ("slice_type", ctypes.c_int32), ("slice_qp", ctypes.c_int32)]


class JmhCabacSliceBytes(ctypes.Structure):
    _fields_ = [("offset", ctypes.c_int64), ("nbytes", ctypes.c_int64), ("nbins", ctypes.c_int64)]


JMC_MB_MAX_BINS = 18944          # csrc/jmh_cabac_write.h: the worst case of one macroblock, in bins
_SIGS_CABAC = {
    "jmh_cabac_write_slices": (_I, [_P, _I, _P, _P, ctypes.c_size_t, _P]),
    "jmh_cabac_write_results": (_I, [_P, _P, _I, _P, _P, ctypes.c_size_t, _P]),
}
EXPORTED_CABAC = tuple(_SIGS_CABAC)


def cabac_max_bytes(nmb, nslices):
    """csrc/jmh_cabac_write.h: JMC_SLICE_MAX_BYTES of every slice at JMC_MB_MAX_BINS per macroblock."""
    return (7 * nmb * JMC_MB_MAX_BINS + 9 * nslices) // 8 + nslices


def cabac_slice_descs(nmb, slice_type, qp, mbs_per_slice=0):
    """Raster runs of mbs_per_slice macroblocks (0: one slice) covering nmb macroblocks, as a
    JmhCabacSliceDesc array; qp: the slice QP, or a sequence of them, cycled."""
    step = mbs_per_slice if mbs_per_slice > 0 else nmb
    firsts = list(range(0, nmb, step))
    qps = [qp] if isinstance(qp, int) else list(qp)
    d = (JmhCabacSliceDesc * len(firsts))()
    for i, f in enumerate(firsts):
        d[i] = JmhCabacSliceDesc(f, min(step, nmb - f), slice_type, qps[i % len(qps)])
    return d


# ---- coded pictures (include/jmhip_coded.h; additive to ABI 14) ----
class JmhCodedSlice(ctypes.Structure):
    _fields_ = [("first_mb", ctypes.c_int32), ("n_mb", ctypes.c_int32), ("slice_type", ctypes.c_int32), ("slice_qp", ctypes.c_int32),
                ("lead_nbits", ctypes.c_int32), ("lead_bits", ctypes.c_uint32)]


class JmhCodedBytes(ctypes.Structure):
    _fields_ = [("offset", ctypes.c_int64), ("nbytes", ctypes.c_int64), ("nbits", ctypes.c_int64), ("nbins", ctypes.c_int64)]


class JmhCodedStats(ctypes.Structure):
    _fields_ = [("ssd", ctypes.c_uint64 * 3), ("fallback", ctypes.c_int32), ("reserved", ctypes.c_int32)]


_SIGS_CODED = {
    "jmh_frame_push_coded": (_I, [_P, _P, _P, _P, _I, _I, ctypes.POINTER(JmhFrameParams), _I, _P, _I, _I]),
    "jmh_frame_push_coded_u16": (_I, [_P, _P, _P, _P, _I, _I, ctypes.POINTER(JmhFrameParams), _I, _P, _I, _I]),
    "jmh_frame_pop_coded": (_I, [_P, _P, ctypes.c_size_t, _P, _P]),
    "jmh_coded_ring_entries": (_I, [_P]),
}
EXPORTED_CODED = tuple(_SIGS_CODED)


# ---- one CABAC slice on many waves (include/jmhip_cabac_split.h; additive to ABI 14) ----
class JmhCabacSplitInfo(ctypes.Structure):
    _fields_ = [("chunk_bins", ctypes.c_int32), ("reserved", ctypes.c_int32), ("chunks", ctypes.c_int64),
                ("longest_slice_chunks", ctypes.c_int64), ("scratch_bytes", ctypes.c_int64)]


_SIGS_CABAC_SPLIT = {
    "jmh_cabac_set_split": (_I, [_P, _I]),
    "jmh_cabac_get_split": (_I, [_P]),
    "jmh_cabac_split_stats": (_I, [_P, _P]),
}
EXPORTED_CABAC_SPLIT = tuple(_SIGS_CABAC_SPLIT)


# ---- pictures that are already on the device (include/jmhip_input.h; additive to ABI 14) ----
JMH_PIX_I420, JMH_PIX_NV12, JMH_PIX_I010, JMH_PIX_P010 = 0, 1, 2, 3


class JmhDevicePicture(ctypes.Structure):
    _fields_ = [("format", ctypes.c_int32), ("width", ctypes.c_int32), ("height", ctypes.c_int32),
                ("plane", ctypes.c_void_p * 3), ("stride", ctypes.c_int64 * 3), ("stream", ctypes.c_void_p)]


_SIGS_INPUT = {
    "jmh_frame_push_device": (_I, [_P, _P, ctypes.POINTER(JmhFrameParams)]),
    "jmh_frame_push_coded_device": (_I, [_P, _P, ctypes.POINTER(JmhFrameParams), _I, _P, _I, _I]),
    "jmh_ingest_picture": (_I, [_P, _P, _P, _P, _P, _I, _I]),
    "jmh_device_input_wait": (_I, [_P]),
    "jmh_device_input_clamped": (_I, [_P, _P]),
    "jmh_device_malloc": (_I, [_P, ctypes.c_size_t, _P]),
    "jmh_device_free": (_I, [_P, _P]),
    "jmh_device_upload": (_I, [_P, _P, _P, ctypes.c_size_t, _P]),
    "jmh_device_stream_create": (_I, [_P, _P]),
    "jmh_device_stream_destroy": (_I, [_P, _P]),
}
EXPORTED_INPUT = tuple(_SIGS_INPUT)


# ---- NAL units finished on the device (include/jmhip_nal.h; additive to ABI 14) ----
JMH_NAL_HEAD_MAX = 64


class JmhNalHead(ctypes.Structure):
    _fields_ = [("nal_ref_idc", ctypes.c_int32), ("nal_unit_type", ctypes.c_int32), ("nbytes", ctypes.c_int32),
                ("bytes", ctypes.c_uint8 * JMH_NAL_HEAD_MAX)]


class JmhNalRange(ctypes.Structure):
    _fields_ = [("offset", ctypes.c_int64), ("nbytes", ctypes.c_int64)]


_SIGS_NAL = {
    "jmh_nal_geometry": (_I, [_P, _P]),
    "jmh_nal_wrap": (_I, [_P, _I, _P, _P, _P, ctypes.c_int64, _P, ctypes.c_size_t, _P, _P]),
    "jmh_coded_nal_heads": (_I, [_P, _I, _P]),
}
EXPORTED_NAL = tuple(_SIGS_NAL)


# ---- RGB pictures pushed from the device (include/jmhip_rgb.h; additive to ABI 14) ----
JMH_PIX_BGRA8, JMH_PIX_RGBA8, JMH_PIX_RGB10A2, JMH_PIX_BGR10A2 = 16, 17, 18, 19
JMH_PIX_BT709, JMH_PIX_FULL_RANGE = 1 << 8, 1 << 9

_SIGS_RGB = {
    "jmh_rgb_coefficients": (_I, [_I, _I, _P]),
}
EXPORTED_RGB = list(_SIGS_RGB)

# ---- 4:2:2 and 4:4:4 pictures pushed from the device (include/jmhip_yuv.h; additive to ABI 14, no entry point) ----
JMH_PIX_I422, JMH_PIX_NV16, JMH_PIX_YUYV, JMH_PIX_UYVY, JMH_PIX_I444, JMH_PIX_VUYA8 = 32, 33, 34, 35, 36, 37
JMH_PIX_I210, JMH_PIX_P210, JMH_PIX_Y210, JMH_PIX_I410, JMH_PIX_Y410 = 40, 41, 42, 43, 44
JMH_PIX_CHROMA_LEFT = 1 << 10
YUV_FORMATS = (JMH_PIX_I422, JMH_PIX_NV16, JMH_PIX_YUYV, JMH_PIX_UYVY, JMH_PIX_I444, JMH_PIX_VUYA8,
               JMH_PIX_I210, JMH_PIX_P210, JMH_PIX_Y210, JMH_PIX_I410, JMH_PIX_Y410)
YUV_444 = (JMH_PIX_I444, JMH_PIX_VUYA8, JMH_PIX_I410, JMH_PIX_Y410)

# ---- RGB tensors pushed from the device (include/jmhip_tensor.h; additive to ABI 14) ----
JMH_T_U8, JMH_T_U16, JMH_T_F16, JMH_T_BF16, JMH_T_F32 = 0, 1, 2, 3, 4
TENSOR_ELEM_BYTES = {JMH_T_U8: 1, JMH_T_U16: 2, JMH_T_F16: 2, JMH_T_BF16: 2, JMH_T_F32: 4}


class JmhDeviceTensor(ctypes.Structure):
    _fields_ = [("dtype", ctypes.c_int32), ("flags", ctypes.c_int32), ("width", ctypes.c_int32), ("height", ctypes.c_int32),
                ("chan", ctypes.c_void_p * 3), ("stride_x", ctypes.c_int64), ("stride_y", ctypes.c_int64), ("stream", ctypes.c_void_p)]


_SIGS_TENSOR = {
    "jmh_frame_push_tensor": (_I, [_P, _P, ctypes.POINTER(JmhFrameParams)]),
    "jmh_frame_push_coded_tensor": (_I, [_P, _P, ctypes.POINTER(JmhFrameParams), _I, _P, _I, _I]),
    "jmh_ingest_tensor": (_I, [_P, _P, _P, _P, _P, _I, _I]),
    "jmh_tensor_quantise": (_I, [_I, _I, _P, ctypes.c_size_t, _P]),
}
EXPORTED_TENSOR = list(_SIGS_TENSOR)

# ---- decoded pictures pulled on the device (include/jmhip_output.h; additive to ABI 14) ----
JMH_OUT_DEBLOCKED, JMH_OUT_RECON = 0, 1


class JmhDevicePictureOut(ctypes.Structure):
    _fields_ = JmhDevicePicture._fields_


class JmhDeviceTensorOut(ctypes.Structure):
    _fields_ = JmhDeviceTensor._fields_


_SIGS_OUTPUT = {
    "jmh_pull_picture": (_I, [_P, _I, _P]),
    "jmh_pull_tensor": (_I, [_P, _I, _P]),
    "jmh_convert_picture": (_I, [_P, _P, _P, _P, _I, _I, _P]),
    "jmh_convert_tensor": (_I, [_P, _P, _P, _P, _I, _I, _P]),
    "jmh_device_output_wait": (_I, [_P]),
    "jmh_device_download": (_I, [_P, _P, _P, ctypes.c_size_t, _P]),
    "jmh_yuv_coefficients": (_I, [_I, _I, _P]),
    "jmh_tensor_dequantise": (_I, [_I, _I, _P, ctypes.c_size_t, _P]),
}
EXPORTED_OUTPUT = tuple(_SIGS_OUTPUT)

# ---- device pushes scaled to a chosen size (include/jmhip_scale.h; additive to ABI 14) ----
JMH_SCALE_OFF, JMH_SCALE_BILINEAR, JMH_SCALE_BICUBIC, JMH_SCALE_LANCZOS3 = 0, 1, 2, 3
JMH_SCALE_CHROMA_LEFT = 1
JMH_SCALE_TAPS_MAX, JMH_SCALE_SRC_MAX = 24, 8192


class JmhScale(ctypes.Structure):
    _fields_ = [("filter", ctypes.c_int32), ("flags", ctypes.c_int32), ("out_width", ctypes.c_int32), ("out_height", ctypes.c_int32)]


_SIGS_SCALE = {
    "jmh_input_scale": (_I, [_P, _P]),
    "jmh_scale_taps": (_I, [_I, _I, _I, _I, _P, _P, _P]),
    "jmh_scale_info": (_I, [_P, _P, _P]),
}
EXPORTED_SCALE = tuple(_SIGS_SCALE)

# ---- the unit seam of the searches' spiral decode (include/jmhip_spiral.h; additive to ABI 14);
#      bound where it is called (Encoder.spiral_positions), so that a library built before it loads
_SIGS_SPIRAL = {
    "jmh_spiral_positions": (_I, [_P, _I, _P]),
}
EXPORTED_SPIRAL = tuple(_SIGS_SPIRAL)


def scale_taps(n_src, n_dst, filter, chroma_left=False):
    """jmh_scale_taps: the tap tables of one axis of the scaler (include/jmhip_scale.h) as (first, taps):
    first[n_dst] int32, unclamped, and taps[n_dst, T] int16, every row summing to 16384.  Needs no
    device.  More than JMH_SCALE_TAPS_MAX taps: JmhError with status JMH_E_UNSUPPORTED_CFG."""
    lib = load()
    nt = ctypes.c_int(0)
    st = lib.jmh_scale_taps(n_src, n_dst, filter, int(bool(chroma_left)), None, None, ctypes.byref(nt))
    _check(st, "jmh_scale_taps")
    first = np.empty(n_dst, np.int32)
    taps = np.empty((n_dst, nt.value), np.int16)
    _check(lib.jmh_scale_taps(n_src, n_dst, filter, int(bool(chroma_left)), _ptr(first), _ptr(taps), ctypes.byref(nt)), "jmh_scale_taps")
    return first, taps


def rgb_coefficients(format, bit_depth):
    """jmh_rgb_coefficients: the conversion of an RGB format with its flags at a bit depth, as 12
    ints: cyr cyg cyb, cur cug cub, cvr cvg cvb, then Yo, Co and maxv.  Needs no device."""
    out = (ctypes.c_int32 * 12)()
    _check(load().jmh_rgb_coefficients(format, bit_depth, out), "jmh_rgb_coefficients")
    return [int(v) for v in out]


def _tensor_dtype(a, dtype=None):
    """The JMH_T_* of a numpy array: from its dtype, unless given (bfloat16 travels as its uint16 bits)."""
    if dtype is not None:
        if a.dtype.itemsize != TENSOR_ELEM_BYTES[dtype]:
            raise ValueError(f"elements of {a.dtype.itemsize} bytes do not hold dtype {dtype}")
        return dtype
    for np_dt, t in ((np.uint8, JMH_T_U8), (np.uint16, JMH_T_U16), (np.float16, JMH_T_F16), (np.float32, JMH_T_F32)):
        if a.dtype == np_dt:
            return t
    raise ValueError(f"no tensor dtype for numpy {a.dtype} (uint8, uint16, float16, float32; bfloat16 as uint16 bits with dtype=JMH_T_BF16)")


def tensor_quantise(array_or_bits, dtype, bit_depth):
    """jmh_tensor_quantise: the integer components in [0, 2^bit_depth - 1] of the elements of a numpy
    array (any shape; a float16 / float32 array, or the elements' bits as uint16 / uint32, which is how
    bfloat16 travels), as int32 of the same shape.  Needs no device."""
    a = np.ascontiguousarray(array_or_bits)
    if a.dtype.itemsize != TENSOR_ELEM_BYTES.get(dtype, a.dtype.itemsize):
        raise ValueError(f"elements of {a.dtype.itemsize} bytes do not hold dtype {dtype}")
    q = np.empty(a.shape, np.int32)
    _check(load().jmh_tensor_quantise(dtype, bit_depth, _ptr(a), a.size, _ptr(q)), "jmh_tensor_quantise")
    return q


def nal_geometry():
    """jmh_nal_geometry: (tile_bytes, chunk_bytes) of the NAL kernels.  Needs no device."""
    t, c = ctypes.c_int(), ctypes.c_int()
    _check(load().jmh_nal_geometry(ctypes.byref(t), ctypes.byref(c)), "jmh_nal_geometry")
    return t.value, c.value


def nal_heads(heads):
    """A JmhNalHead array from (nal_ref_idc, nal_unit_type, bytes) triples; a head holds at most
    JMH_NAL_HEAD_MAX bytes."""
    a = (JmhNalHead * len(heads))()
    for i, (ref_idc, typ, data) in enumerate(heads):
        data = bytes(data)
        if len(data) > JMH_NAL_HEAD_MAX:
            raise ValueError(f"head {i}: {len(data)} bytes exceed JMH_NAL_HEAD_MAX")
        a[i].nal_ref_idc, a[i].nal_unit_type, a[i].nbytes = ref_idc, typ, len(data)
        ctypes.memmove(a[i].bytes, data, len(data))
    return a


def _addr(p):
    """A device address: an int, or any object with data_ptr() (a torch tensor, for one; for a whole
    descriptor of one, with its stream, see Encoder.from_torch)."""
    return int(p.data_ptr()) if hasattr(p, "data_ptr") else int(p)


class DevicePicture:
    """jmh_device_picture: format (JMH_PIX_*), the source size in luma samples, the planes' device
    addresses (ints or objects with data_ptr(); two for NV12 / P010), their strides in bytes, and
    the stream (Encoder.device_stream, or None) on which the planes are complete."""

    def __init__(self, format, width, height, planes, strides, stream=None):
        self.format, self.width, self.height = format, width, height
        self.planes, self.strides, self.stream = list(planes), list(strides), stream

    def struct(self):
        s = JmhDevicePicture(self.format, self.width, self.height)
        for i, (p, st) in enumerate(zip(self.planes, self.strides)):
            s.plane[i] = _addr(p) if p is not None else None
            s.stride[i] = st
        s.stream = self.stream
        return s


class HostLayout:
    """What to_device and to_device_rgb lay out: buf (uint8, to be uploaded as one block), the planes' byte offsets
    in it and their strides."""

    def __init__(self, format, width, height, buf, offsets, strides):
        self.format, self.width, self.height, self.buf, self.offsets, self.strides = format, width, height, buf, offsets, strides

    def at(self, base, stream=None):
        """The DevicePicture of this layout uploaded at device address base."""
        return DevicePicture(self.format, self.width, self.height, [_addr(base) + o for o in self.offsets], self.strides, stream)


def to_device(pics, format, pad_stride=0, misalign=0):
    """A numpy picture pics = (y, u, v) of the source size (h x w, h/2 x w/2 twice) laid out in the
    requested format as a HostLayout.  pad_stride: bytes added to every row (filled with 0xA5, as
    is everything between the planes); misalign: the offset in bytes of every plane's first sample
    from a 256-byte boundary of the block.  P010 gets noise in the low 6 bits of every word."""
    wide, semi = format >= JMH_PIX_I010, format in (JMH_PIX_NV12, JMH_PIX_P010)
    dt = np.uint16 if wide else np.uint8
    y, u, v = (np.ascontiguousarray(a, dt) for a in pics)
    h, w = y.shape
    if format == JMH_PIX_P010:
        noise = lambda a: (np.arange(a.size, dtype=np.uint32).reshape(a.shape) * 37 + 11) & 63
        y, u, v = ((a.astype(np.uint32) << 6 | noise(a)).astype(np.uint16) for a in (y, u, v))
    if semi:
        uv = np.empty((h // 2, w), dt)
        uv[:, 0::2], uv[:, 1::2] = u, v
        planes = [y, uv]
    else:
        planes = [y, u, v]
    offsets, strides, end = [], [], 0
    for a in planes:
        rb = a.shape[1] * a.itemsize
        offsets.append((end + 255) // 256 * 256 + misalign)
        strides.append(rb + pad_stride)
        end = offsets[-1] + (a.shape[0] - 1) * strides[-1] + rb      # no byte behind the last row's samples
    buf = np.full(end, 0xA5, np.uint8)
    for a, o, st in zip(planes, offsets, strides):
        rb = a.shape[1] * a.itemsize
        rows = np.lib.stride_tricks.as_strided(buf[o:], (a.shape[0], rb), (st, 1))
        rows[:] = a.view(np.uint8).reshape(a.shape[0], rb)
    return HostLayout(format, w, h, buf, offsets, strides)


def to_device_rgb(array, format, pad_stride=0, misalign=0):
    """An RGB picture laid out as a one-plane HostLayout: array is (h, w, 4) uint8 (the bytes of every
    pixel in memory order) or (h, w) uint32 (the packed words), format one of JMH_PIX_BGRA8 ..
    JMH_PIX_BGR10A2 with its flags.  pad_stride: bytes added to every row (a multiple of 4, filled
    with 0xA5); misalign: the offset in bytes of the first pixel from a 256-byte boundary of the
    block (a multiple of 4).  Nothing lies behind the last row's 4 * w bytes."""
    a = np.ascontiguousarray(array)
    if a.dtype == np.uint32 and a.ndim == 2:
        a = a.astype("<u4").view(np.uint8).reshape(a.shape[0], a.shape[1], 4)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 4:
        raise ValueError("to_device_rgb takes an (h, w, 4) uint8 or an (h, w) uint32 array")
    if misalign % 4 or pad_stride % 4:
        raise ValueError("misalign and pad_stride are multiples of 4: a pixel is a dword")
    h, w = a.shape[:2]
    rb = 4 * w
    stride = rb + pad_stride
    buf = np.full(misalign + (h - 1) * stride + rb, 0xA5, np.uint8)
    rows = np.lib.stride_tricks.as_strided(buf[misalign:], (h, rb), (stride, 1))
    rows[:] = a.reshape(h, rb)
    return HostLayout(format, w, h, buf, [misalign], [stride])


def to_device_yuv(planes, format, pad_stride=0, misalign=0):
    """A 4:2:2 or 4:4:4 numpy picture planes = (y, u, v) laid out in the requested format of
    include/jmhip_yuv.h (JMH_PIX_I422 .. JMH_PIX_Y410, JMH_PIX_CHROMA_LEFT allowed) as a HostLayout.
    y is h x w; u and v are h x w/2 for the 4:2:2 formats and h x w for the 4:4:4 ones.  The packed
    layouts are interleaved here.  pad_stride, misalign: as for to_device (the formats of 16-bit words
    want them even, VUYA8 and Y410 multiples of 4; this function does not insist, so that a test can
    build what the library must refuse).  P210 and Y210 get noise in the low 6 bits of every word,
    VUYA8 and Y410 in their alpha."""
    layout = format & ~JMH_PIX_CHROMA_LEFT
    if layout not in YUV_FORMATS:
        raise ValueError(f"to_device_yuv: format {format} is not one of include/jmhip_yuv.h")
    dt = np.uint16 if layout >= JMH_PIX_I210 else np.uint8
    y, u, v = (np.ascontiguousarray(a, dt) for a in planes)
    h, w = y.shape
    if u.shape != v.shape or u.shape != (h, w if layout in YUV_444 else w // 2):
        raise ValueError("to_device_yuv: the chroma planes do not have the format's size")
    noise = lambda a, m: (np.arange(a.size, dtype=np.uint32).reshape(a.shape) * 37 + 11) & m
    if layout in (JMH_PIX_P210, JMH_PIX_Y210):
        y, u, v = ((a.astype(np.uint32) << 6 | noise(a, 63)).astype(np.uint16) for a in (y, u, v))
    if layout in (JMH_PIX_I422, JMH_PIX_I444, JMH_PIX_I210, JMH_PIX_I410):
        src = [y, u, v]
    elif layout in (JMH_PIX_NV16, JMH_PIX_P210):
        uv = np.empty((h, w), dt)
        uv[:, 0::2], uv[:, 1::2] = u, v
        src = [y, uv]
    elif layout in (JMH_PIX_YUYV, JMH_PIX_UYVY, JMH_PIX_Y210):
        p = np.empty((h, 2 * w), dt)
        o = 1 if layout == JMH_PIX_UYVY else 0                          # where Y0 lies in Y0 U Y1 V / U Y0 V Y1
        p[:, o::4], p[:, o + 2::4] = y[:, 0::2], y[:, 1::2]
        p[:, 1 - o::4], p[:, 3 - o::4] = u, v
        src = [p]
    elif layout == JMH_PIX_VUYA8:
        p = np.empty((h, w, 4), np.uint8)
        p[..., 0], p[..., 1], p[..., 2], p[..., 3] = v, u, y, noise(y, 255)
        src = [p.reshape(h, 4 * w)]
    else:                                                               # Y410
        p = u.astype(np.uint32) | y.astype(np.uint32) << 10 | v.astype(np.uint32) << 20 | noise(y, 3) << 30
        src = [p.astype("<u4")]
    offsets, strides, end = [], [], 0
    for a in src:
        rb = a.shape[1] * a.itemsize
        offsets.append((end + 255) // 256 * 256 + misalign)
        strides.append(rb + pad_stride)
        end = offsets[-1] + (a.shape[0] - 1) * strides[-1] + rb      # no byte behind the last row's samples
    buf = np.full(end, 0xA5, np.uint8)
    for a, o, st in zip(src, offsets, strides):
        rb = a.shape[1] * a.itemsize
        rows = np.lib.stride_tricks.as_strided(buf[o:], (a.shape[0], rb), (st, 1))
        rows[:] = np.ascontiguousarray(a).view(np.uint8).reshape(a.shape[0], rb)
    return HostLayout(format, w, h, buf, offsets, strides)


def yuv_reduce(y, u, v, format, bit_depth):
    """The numpy reference of include/jmhip_yuv.h: the planar 4:2:2 or 4:4:4 samples (as given to
    to_device_yuv) reduced to the 4:2:0 picture (y, u, v) of the source size, in exact integers.
    Samples of I210 / I410 above maxv are taken as maxv first; luma is copied; chroma is
    (C[2j][i] + C[2j+1][i] + 1) >> 1 for 4:2:2, the rounded mean of the 2x2 block for 4:4:4, and with
    JMH_PIX_CHROMA_LEFT h(r) = C[r][max(2i-1, 0)] + 2 C[r][2i] + C[r][2i+1], (h(2j) + h(2j+1) + 4) >> 3."""
    layout = format & ~JMH_PIX_CHROMA_LEFT
    if layout not in YUV_FORMATS:
        raise ValueError(f"yuv_reduce: format {format} is not one of include/jmhip_yuv.h")
    dt = np.uint16 if bit_depth > 8 else np.uint8
    y, u, v = (np.asarray(a).astype(np.int64) for a in (y, u, v))
    if layout in (JMH_PIX_I210, JMH_PIX_I410):
        y, u, v = (np.minimum(a, (1 << bit_depth) - 1) for a in (y, u, v))

    def chroma(c):
        if layout not in YUV_444:
            return (c[0::2] + c[1::2] + 1) >> 1
        if not format & JMH_PIX_CHROMA_LEFT:
            return (c[0::2, 0::2] + c[0::2, 1::2] + c[1::2, 0::2] + c[1::2, 1::2] + 2) >> 2
        left = np.concatenate([c[:, :1], c[:, 1:-1:2]], axis=1)         # C[r][max(2i - 1, 0)]
        hs = left + 2 * c[:, 0::2] + c[:, 1::2]
        return (hs[0::2] + hs[1::2] + 4) >> 3
    return y.astype(dt), chroma(u).astype(dt), chroma(v).astype(dt)


class DeviceTensor:
    """jmh_device_tensor over addresses you own: dtype (JMH_T_*), flags (JMH_PIX_BT709 |
    JMH_PIX_FULL_RANGE), the size in pixels, the device addresses of R, G and B at pixel (0, 0) (ints or
    objects with data_ptr()), the bytes between pixels and between rows, and the stream on which the
    elements are complete (or None)."""

    def __init__(self, dtype, flags, width, height, chans, stride_x, stride_y, stream=None):
        self.dtype, self.flags, self.width, self.height = dtype, flags, width, height
        self.chans, self.stride_x, self.stride_y, self.stream = list(chans), stride_x, stride_y, stream

    def struct(self):
        s = JmhDeviceTensor(self.dtype, self.flags, self.width, self.height)
        for i, p in enumerate(self.chans):
            s.chan[i] = _addr(p) if p is not None else None
        s.stride_x, s.stride_y, s.stream = self.stride_x, self.stride_y, self.stream
        return s


class TensorLayout:
    """What to_device_tensor lays out: buf (uint8, to be uploaded as one block), the byte offsets of
    R, G and B at pixel (0, 0) in it, and the two strides."""

    def __init__(self, dtype, flags, width, height, buf, offsets, stride_x, stride_y):
        self.dtype, self.flags, self.width, self.height = dtype, flags, width, height
        self.buf, self.offsets, self.stride_x, self.stride_y = buf, offsets, stride_x, stride_y

    def at(self, base, stream=None):
        """The DeviceTensor of this layout uploaded at device address base."""
        return DeviceTensor(self.dtype, self.flags, self.width, self.height, [_addr(base) + o for o in self.offsets], self.stride_x,
                            self.stride_y, stream)


def to_device_tensor(array, layout="chw", order="rgb", flags=0, pad_stride=0, misalign=0, dtype=None):
    """An RGB tensor laid out as a TensorLayout.  array: (C, h, w) for layout "chw" with C = 3, or
    (h, w, C) for "hwc" with C = 3 or 4, of uint8, uint16, float16 or float32 (bfloat16: its uint16
    bits with dtype=JMH_T_BF16).  order: which channel of the array is which component, "rgb",
    "bgr", "gbr", ... (a fourth channel of "hwc" is never read).  pad_stride: bytes added to every row
    (a multiple of the element size, filled with 0xA5); misalign: the offset in bytes of every
    channel's base from a 256-byte boundary of the block (a multiple of the element size).  Nothing
    lies behind the last element read of the last row."""
    a = np.ascontiguousarray(array)
    dt = _tensor_dtype(a, dtype)
    es = TENSOR_ELEM_BYTES[dt]
    if a.ndim != 3 or layout not in ("chw", "hwc") or sorted(order) != ["b", "g", "r"]:
        raise ValueError("to_device_tensor takes a 3-D array, layout 'chw' or 'hwc' and an order that is a permutation of 'rgb'")
    if misalign % es or pad_stride % es:
        raise ValueError("misalign and pad_stride are multiples of the element size")
    where = [order.index(c) for c in "rgb"]                   # the array's channel of R, G, B
    raw = a.view(np.uint8)
    if layout == "chw":
        C, h, w = a.shape
        if C != 3:
            raise ValueError("layout 'chw' takes (3, h, w)")
        rb = w * es
        stride_y = rb + pad_stride
        starts, end = [], 0
        for _ in range(3):
            starts.append((end + 255) // 256 * 256 + misalign)
            end = starts[-1] + (h - 1) * stride_y + rb          # no byte behind the last row's elements
        buf = np.full(end, 0xA5, np.uint8)
        for c in range(3):
            rows = np.lib.stride_tricks.as_strided(buf[starts[c]:], (h, rb), (stride_y, 1))
            rows[:] = raw[c].reshape(h, rb)
        return TensorLayout(dt, flags, w, h, buf, [starts[c] for c in where], es, stride_y)
    h, w, C = a.shape
    if C not in (3, 4):
        raise ValueError("layout 'hwc' takes (h, w, 3) or (h, w, 4)")
    rb = w * C * es
    stride_y = rb + pad_stride
    end = misalign + (h - 1) * stride_y + ((w - 1) * C + 3) * es   # the last pixel's three channels, not its fourth
    buf = np.full(misalign + (h - 1) * stride_y + rb, 0xA5, np.uint8)
    rows = np.lib.stride_tricks.as_strided(buf[misalign:], (h, rb), (stride_y, 1))
    rows[:] = raw.reshape(h, rb)
    return TensorLayout(dt, flags, w, h, buf[:end].copy(), [misalign + c * es for c in where], C * es, stride_y)


def yuv_coefficients(flags, bit_depth):
    """jmh_yuv_coefficients: the inverse conversion of the flags (JMH_PIX_BT709 | JMH_PIX_FULL_RANGE) at
    a bit depth of 8 or 10, as 8 ints: iy, irv, igu, igv, ibu, then Yo, Co and M.  Needs no device."""
    out = (ctypes.c_int32 * 8)()
    _check(load().jmh_yuv_coefficients(flags, bit_depth, out), "jmh_yuv_coefficients")
    return [int(v) for v in out]


_TENSOR_STORAGE = {JMH_T_U8: np.uint8, JMH_T_U16: np.uint16, JMH_T_F16: np.float16, JMH_T_BF16: np.uint16, JMH_T_F32: np.float32}


def tensor_dequantise(q, dtype, bit_depth):
    """jmh_tensor_dequantise: the elements that hold the integer components q (any shape, clamped to
    [0, 2^bit_depth - 1]) as a numpy array of the same shape: uint8, uint16, float16 or float32;
    bfloat16 comes as its uint16 bits.  Needs no device."""
    q = np.ascontiguousarray(q, np.int32)
    out = np.empty(q.shape, _TENSOR_STORAGE[dtype])
    _check(load().jmh_tensor_dequantise(dtype, bit_depth, _ptr(q), q.size, _ptr(out)), "jmh_tensor_dequantise")
    return out


class DevicePictureOut(DevicePicture):
    """jmh_device_picture_out: a DevicePicture whose planes the library writes (Encoder.pull / convert);
    stream: the stream the pull is queued on, or None for a picture that is complete on return."""

    def struct(self):
        s = JmhDevicePictureOut()
        ctypes.memmove(ctypes.byref(s), ctypes.byref(DevicePicture.struct(self)), ctypes.sizeof(s))
        return s


class DeviceTensorOut(DeviceTensor):
    """jmh_device_tensor_out: a DeviceTensor whose channels the library writes (Encoder.pull_tensor /
    convert_tensor)."""

    def struct(self):
        s = JmhDeviceTensorOut()
        ctypes.memmove(ctypes.byref(s), ctypes.byref(DeviceTensor.struct(self)), ctypes.sizeof(s))
        return s


def _rows_view(buf, offset, rows, row_bytes, stride):
    return np.lib.stride_tricks.as_strided(buf[offset:], (rows, row_bytes), (stride, 1))


class OutLayout:
    """What out_layout lays out: a destination of nbytes bytes, the planes' byte offsets in it and
    their strides.  at(base) is its DevicePictureOut at a device address; planes(buf) reads the
    picture out of the block's bytes; mask() marks the bytes that are destination elements."""

    def __init__(self, format, width, height, nbytes, offsets, strides, shapes, itemsize):
        self.format, self.width, self.height, self.nbytes = format, width, height, nbytes
        self.offsets, self.strides, self.shapes, self.itemsize = offsets, strides, shapes, itemsize

    def at(self, base, stream=None):
        return DevicePictureOut(self.format, self.width, self.height, [_addr(base) + o for o in self.offsets], self.strides, stream)

    def planes(self, buf):
        """the planes as arrays: (y, u, v), (y, uv) of NV12 / P010, or one (h, w) uint32 array of RGB"""
        buf = np.ascontiguousarray(buf, np.uint8)
        dt = {1: np.uint8, 2: np.uint16, 4: np.uint32}[self.itemsize]
        return [_rows_view(buf, o, r, n * self.itemsize, st).copy().view(dt) for o, st, (r, n) in zip(self.offsets, self.strides, self.shapes)]

    def mask(self):
        m = np.zeros(self.nbytes, bool)
        for o, st, (r, n) in zip(self.offsets, self.strides, self.shapes):
            _rows_view(m, o, r, n * self.itemsize, st)[:] = True
        return m


def out_layout(format, width, height, pad_stride=0, misalign=0, guard=0):
    """A destination for Encoder.pull / convert in a format of jmhip_input.h or jmhip_rgb.h (with its
    flags), as an OutLayout.  pad_stride: bytes added to every row; misalign: the offset in bytes
    of every plane's first element from a 256-byte boundary of the block; guard: bytes of the block
    in front of the first plane (rounded up to that boundary) and behind the last element."""
    lay = format & ~(JMH_PIX_BT709 | JMH_PIX_FULL_RANGE)
    if lay >= JMH_PIX_BGRA8:
        es, shapes = 4, [(height, width)]
    else:
        es = 2 if lay >= JMH_PIX_I010 else 1
        shapes = [(height, width), (height // 2, width)] if lay in (JMH_PIX_NV12, JMH_PIX_P010) else \
            [(height, width), (height // 2, width // 2), (height // 2, width // 2)]
    offsets, strides, end = [], [], guard
    for r, n in shapes:
        offsets.append((end + 255) // 256 * 256 + misalign)
        strides.append(n * es + pad_stride)
        end = offsets[-1] + (r - 1) * strides[-1] + n * es
    return OutLayout(format, width, height, end + guard, offsets, strides, shapes, es)


class OutTensorLayout:
    """What out_tensor_layout lays out: a destination of nbytes bytes, the byte offsets of R, G and B
    at pixel (0, 0) in it and the two strides.  at(base) is its DeviceTensorOut; channels(buf) reads
    R, G, B (h x w each, bfloat16 as uint16 bits) out of the block's bytes; mask() marks the bytes that
    are destination elements."""

    def __init__(self, dtype, flags, width, height, nbytes, offsets, stride_x, stride_y):
        self.dtype, self.flags, self.width, self.height, self.nbytes = dtype, flags, width, height, nbytes
        self.offsets, self.stride_x, self.stride_y = offsets, stride_x, stride_y

    def at(self, base, stream=None):
        return DeviceTensorOut(self.dtype, self.flags, self.width, self.height, [_addr(base) + o for o in self.offsets], self.stride_x,
                               self.stride_y, stream)

    def _view(self, buf, offset):
        es = TENSOR_ELEM_BYTES[self.dtype]
        return np.lib.stride_tricks.as_strided(buf[offset:], (self.height, self.width, es), (self.stride_y, self.stride_x, 1))

    def channels(self, buf):
        buf = np.ascontiguousarray(buf, np.uint8)
        return [np.ascontiguousarray(self._view(buf, o)).view(_TENSOR_STORAGE[self.dtype]).reshape(self.height, self.width) for o in self.offsets]

    def mask(self):
        m = np.zeros(self.nbytes, bool)
        for o in self.offsets:
            self._view(m, o)[:] = True
        return m


def out_tensor_layout(dtype, width, height, layout="chw", order="rgb", channels=3, flags=0, pad_stride=0, misalign=0, guard=0):
    """A destination for Encoder.pull_tensor / convert_tensor, as an OutTensorLayout: layout "chw"
    (three planes) or "hwc" with channels 3 or 4 (the fourth is never written); order: which channel
    of the array holds which component ("rgb", "bgr", ...).  pad_stride, misalign (multiples of the
    element size) and guard as for out_layout."""
    es = TENSOR_ELEM_BYTES[dtype]
    if layout not in ("chw", "hwc") or sorted(order) != ["b", "g", "r"] or channels not in (3, 4) or (layout == "chw" and channels != 3):
        raise ValueError("out_tensor_layout takes layout 'chw' or 'hwc', 3 (or for 'hwc' 4) channels and an order that is a permutation of 'rgb'")
    if misalign % es or pad_stride % es:
        raise ValueError("misalign and pad_stride are multiples of the element size")
    where = [order.index(c) for c in "rgb"]
    if layout == "chw":
        stride_y = width * es + pad_stride
        starts, end = [], guard
        for _ in range(3):
            starts.append((end + 255) // 256 * 256 + misalign)
            end = starts[-1] + (height - 1) * stride_y + width * es
        return OutTensorLayout(dtype, flags, width, height, end + guard, [starts[c] for c in where], es, stride_y)
    stride_y = width * channels * es + pad_stride
    start = (guard + 255) // 256 * 256 + misalign
    end = start + (height - 1) * stride_y + ((width - 1) * channels + 3) * es      # the last pixel's three channels
    return OutTensorLayout(dtype, flags, width, height, end + guard, [start + c * es for c in where], channels * es, stride_y)


def pad_to_coded(pics, cw, ch):
    """host/yuv.c jm_pad_picture in numpy: (y, u, v) of the source size replicated to cw x ch."""
    out = []
    for a, (H, W) in zip(pics, ((ch, cw), (ch // 2, cw // 2), (ch // 2, cw // 2))):
        out.append(np.pad(a, ((0, H - a.shape[0]), (0, W - a.shape[1])), mode="edge"))
    return tuple(out)


def coded_slice_descs(nmb, slice_type, qp, mbs_per_slice=0, lead=()):
    """The descriptors of a coded picture (a JmhCodedSlice array), from the two writers' helpers:
    the raster runs and lead bits of slice_descs, the slice QPs of cabac_slice_descs."""
    a, b = slice_descs(nmb, slice_type, mbs_per_slice, lead), cabac_slice_descs(nmb, slice_type, qp, mbs_per_slice)
    d = (JmhCodedSlice * len(a))()
    for i, (x, y) in enumerate(zip(a, b)):
        d[i] = JmhCodedSlice(x.first_mb, x.n_mb, x.slice_type, y.slice_qp, x.lead_nbits, x.lead_bits)
    return d


def coded_from_runs(runs, slice_type, qp, lead=()):
    """The same for slices of the given macroblock counts (raster runs in order)."""
    d = (JmhCodedSlice * len(runs))()
    first = 0
    for i, n in enumerate(runs):
        nb, bits = lead[i % len(lead)] if lead else (0, 0)
        d[i] = JmhCodedSlice(first, n, slice_type, qp, nb, bits & ((1 << nb) - 1))
        first += n
    return d


def split_coded(descs):
    """A JmhCodedSlice array as the synchronous writers take it: (JmhSliceDesc array, JmhCabacSliceDesc array)."""
    a, b = (JmhSliceDesc * len(descs))(), (JmhCabacSliceDesc * len(descs))()
    for i, d in enumerate(descs):
        a[i] = JmhSliceDesc(d.first_mb, d.n_mb, d.slice_type, d.lead_nbits, d.lead_bits)
        b[i] = JmhCabacSliceDesc(d.first_mb, d.n_mb, d.slice_type, d.slice_qp)
    return a, b


class JmhError(RuntimeError):
    status = None                # the JMH_E_* code, where a jmh_* call failed


_lib = None


def load(path=LIB_PATH):
    """Load libjmhip.so (raises if it was not built — the product has no fallback)."""
    global _lib
    if _lib is not None and path == LIB_PATH:
        return _lib
    if not os.path.exists(path):
        raise JmhError(f"libjmhip.so not found at {path}: build it with __graft_entry__.build()")
    lib = ctypes.CDLL(path)
    for name, (res, args) in list(_SIGS.items()) + list(_SIGS_CAVLC.items()) + list(_SIGS_CABAC.items()) + list(_SIGS_CODED.items()) + \
            list(_SIGS_CABAC_SPLIT.items()) + list(_SIGS_INPUT.items()) + list(_SIGS_NAL.items()) + list(_SIGS_RGB.items()) + list(_SIGS_TENSOR.items()) + \
            list(_SIGS_OUTPUT.items()) + list(_SIGS_SCALE.items()):
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    if lib.jmh_abi_version() != JMH_ABI_VERSION:
        raise JmhError(f"{path}: ABI version {lib.jmh_abi_version()} != {JMH_ABI_VERSION} (stale build?)")
    if path == LIB_PATH:
        _lib = lib
    return lib


def _one_hip_runtime():
    """Stream handles and events belong to one HIP runtime.  A process that loaded this library before
    torch can hold two (torch brings its own copy): refuse to pass handles between them."""
    try:
        with open("/proc/self/maps") as f:
            paths = {line.split()[-1] for line in f if "libamdhip64" in line}
    except OSError:
        return
    if len(paths) > 1:
        raise JmhError("two HIP runtimes in this process (" + ", ".join(sorted(paths)) + "): a torch stream cannot be handed to libjmhip.so; "
                       "import torch before jmhip loads its library")


def _check(st, what):
    if st != JMH_OK:
        e = JmhError(f"{what}: {STATUS.get(st, st)} ({st})")
        e.status = st
        raise e


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def make_config(width, height, search_range=32, search_mode=0, use_hadamard=1,
                restrict_search_range=2, inter_search=(1, 1, 1, 1, 1, 1, 1), slots=2, kernel_timing=False,
                pipeline_depth=0, transform_8x8_mode=0, jm_version=8, quant_offset=(682, 342), epzs_dual_refinement=0, slice_mbs=0,
                bit_depth=8, rdo=0, symbol_mode=None, epzs_subpel_me=0, epzs_subpel_thres_scale=0, epzs_min_thres_scale=0,
                epzs_max_thres_scale=0, constrained_intra_pred=0):
    """jm_version >= 10 selects the JM >= 10 quantisation rounding with the flat OffsetMatrix
    entries quant_offset = (I slices, P slices) at OffsetBits 11 (docs/JM_SEMANTICS.md item 45)."""
    cfg = JmhConfig()
    cfg.width, cfg.height = width, height
    cfg.search_range, cfg.search_mode = search_range, search_mode
    cfg.use_hadamard, cfg.restrict_search_range = use_hadamard, restrict_search_range
    for i, v in enumerate(inter_search):
        cfg.inter_search[i + 1] = v
    cfg.num_ref_frames, cfg.constrained_intra_pred, cfg.num_frame_slots = 1, constrained_intra_pred, slots
    cfg.flags = JMH_FLAG_KERNEL_TIMING if kernel_timing else 0
    cfg.pipeline_depth = pipeline_depth
    cfg.transform_8x8_mode = transform_8x8_mode
    cfg.jm_version = jm_version
    cfg.epzs_dual_refinement = epzs_dual_refinement
    cfg.slice_mbs = slice_mbs
    cfg.bit_depth = bit_depth
    cfg.rdo = rdo
    cfg.symbol_mode = (1 if rdo else 0) if symbol_mode is None else symbol_mode
    cfg.epzs_subpel_me, cfg.epzs_subpel_thres_scale = epzs_subpel_me, epzs_subpel_thres_scale
    cfg.epzs_min_thres_scale, cfg.epzs_max_thres_scale = epzs_min_thres_scale, epzs_max_thres_scale
    if jm_version >= 10:
        cfg.quant_offset[0], cfg.quant_offset[1] = quant_offset
    return cfg


def frame_params(slice_type, qp, chroma_qp_offset=0, deblock=None, rdo=0, bit_depth=8):
    """deblock: None (no device deblocking) or (disable_idc, alpha_div2, beta_div2); rdo: fill the
    RDOptimization 1 lambdas."""
    fp = JmhFrameParams()
    fp.slice_type, fp.qp = slice_type, qp
    fp.lambda_mode = fp.lambda_motion = lambda_rdo_off(qp)
    if rdo:
        fp.lambda_rd, fp.lambda_factor_rd = lambda_rdo_on(qp, bit_depth)
    fp.chroma_qp_offset = chroma_qp_offset
    if deblock is not None:
        fp.deblock = 1
        fp.lf_disable, fp.lf_alpha_div2, fp.lf_beta_div2 = deblock
    return fp


def split_yuv(frame, w, h):
    """I420 buffer (w*h*3/2 bytes) -> contiguous (y, u, v) uint8 planes."""
    f = np.ascontiguousarray(frame, dtype=np.uint8).reshape(-1)
    y = f[: w * h].reshape(h, w)
    u = f[w * h: w * h + w * h // 4].reshape(h // 2, w // 2)
    v = f[w * h + w * h // 4:].reshape(h // 2, w // 2)
    return np.ascontiguousarray(y), np.ascontiguousarray(u), np.ascontiguousarray(v)


class Encoder:
    """One jmh_ctx: the macroblock hot path of one video stream on one HIP device."""

    def __init__(self, width, height, device=0, **kw):
        self.lib = load()
        self.w, self.h = width, height
        self.mbw, self.mbh = width // 16, height // 16
        self.cfg = make_config(width, height, **kw)
        # High 10 contexts take 16-bit pictures through the *_u16 entry points
        self.hbd = self.cfg.bit_depth > 8
        self.sfx = "_u16" if self.hbd else ""
        self.pdt = np.uint16 if self.hbd else np.uint8
        ctx = ctypes.c_void_p()
        _check(self.lib.jmh_create(ctypes.byref(self.cfg), device, ctypes.byref(ctx)), "jmh_create")
        self.ctx = ctx

    def close(self):
        if self.ctx:
            self.lib.jmh_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _planes(self, y, u, v):
        return [np.ascontiguousarray(a, self.pdt) for a in (y, u, v)]

    def set_reference(self, y, u, v):
        y, u, v = self._planes(y, u, v)
        fn = "jmh_set_reference" + self.sfx
        _check(getattr(self.lib, fn)(self.ctx, 0, 0, _ptr(y), _ptr(u), _ptr(v), self.w, self.w // 2), fn)

    def encode(self, y, u, v, slice_type, qp, chroma_qp_offset=0, deblock=None):
        fp = frame_params(slice_type, qp, chroma_qp_offset, deblock, self.cfg.rdo, self.cfg.bit_depth)
        y, u, v = self._planes(y, u, v)
        fn = "jmh_frame_submit" + self.sfx
        _check(getattr(self.lib, fn)(self.ctx, _ptr(y), _ptr(u), _ptr(v), self.w, self.w // 2, ctypes.byref(fp)), fn)
        _check(self.lib.jmh_frame_wait(self.ctx), "jmh_frame_wait")
        return self.results(), self.recon()

    # ---- pipelined pictures (jmh_frame_push / jmh_frame_pop) ----
    def push(self, y, u, v, slice_type, qp, chroma_qp_offset=0, deblock=None):
        fp = frame_params(slice_type, qp, chroma_qp_offset, deblock, self.cfg.rdo, self.cfg.bit_depth)
        y, u, v = self._planes(y, u, v)
        fn = "jmh_frame_push" + self.sfx
        _check(getattr(self.lib, fn)(self.ctx, _ptr(y), _ptr(u), _ptr(v), self.w, self.w // 2, ctypes.byref(fp)), fn)

    def pop(self):
        """Wait for the oldest pushed picture; returns (results, recon)."""
        _check(self.lib.jmh_frame_pop(self.ctx), "jmh_frame_pop")
        return self.results(), self.recon()

    # ---- coded pictures (jmh_frame_push_coded / jmh_frame_pop_coded) ----
    def _arm(self, heads):
        """jmh_coded_nal_heads: heads (a JmhNalHead array, see nal_heads, or its triples) for the next coded push."""
        if heads is not None:
            if not isinstance(heads, ctypes.Array):
                heads = nal_heads(heads)
            _check(self.lib.jmh_coded_nal_heads(self.ctx, len(heads), ctypes.cast(heads, _P)), "jmh_coded_nal_heads")

    def nal_wrap(self, heads, payload, where, nbins=0, cap=None):
        """jmh_nal_wrap, the unit seam: heads as for nal_heads, payload bytes, where = [(offset, nbytes)]
        of each unit's payload; nbins > 0 asks for the cabac_zero_words.  Returns (the access unit's
        bytes, [(offset, nbytes)] of each NAL unit in them).  cap: the size of the output buffer; an
        access unit that needs more raises JmhError (JMH_E_INVALID_ARG, .where and .total filled).
        Without cap the buffer grows to the counted size and the call is repeated."""
        if not isinstance(heads, ctypes.Array):
            heads = nal_heads(heads)
        n = len(heads)
        pay = np.frombuffer(bytes(payload), np.uint8) if len(payload) else np.zeros(1, np.uint8)
        wi, wo, total = (JmhNalRange * n)(), (JmhNalRange * n)(), ctypes.c_int64()
        for i, (off, nb) in enumerate(where):
            wi[i].offset, wi[i].nbytes = off, nb
        size = cap if cap is not None else 3 * len(payload) // 2 + n * (2 * JMH_NAL_HEAD_MAX + 5)
        while True:
            out = np.zeros(max(size, 1), np.uint8)
            st = self.lib.jmh_nal_wrap(self.ctx, n, ctypes.cast(heads, _P), _ptr(pay), ctypes.cast(wi, _P), nbins, _ptr(out), size,
                                       ctypes.cast(wo, _P), ctypes.byref(total))
            if st == JMH_E_INVALID_ARG and cap is None and total.value > size:
                size = total.value
                continue
            break
        wl = [(w.offset, w.nbytes) for w in wo]
        if st != JMH_OK:
            e = JmhError(f"jmh_nal_wrap: {STATUS.get(st, st)} ({st})")
            e.status, e.where, e.total = st, wl, total.value
            raise e
        return out[:total.value].tobytes(), wl

    def push_coded(self, y, u, v, slice_type, qp, descs, crop=None, deblock=None, chroma_qp_offset=0, heads=None):
        """jmh_frame_push with the picture's slices (a JmhCodedSlice array, see coded_slice_descs): its
        slice data is written on the device behind its last macroblock.  crop: (width, height) of
        the distortion sums, default the coded size.  heads: one per slice (see nal_heads): the
        picture's pop_coded then returns its NAL units, start codes included."""
        self._arm(heads)
        fp = frame_params(slice_type, qp, chroma_qp_offset, deblock, self.cfg.rdo, self.cfg.bit_depth)
        y, u, v = self._planes(y, u, v)
        cw, ch = crop if crop is not None else (self.w, self.h)
        self._coded_n = getattr(self, "_coded_n", [])
        fn = "jmh_frame_push_coded" + self.sfx
        _check(getattr(self.lib, fn)(self.ctx, _ptr(y), _ptr(u), _ptr(v), self.w, self.w // 2, ctypes.byref(fp), len(descs),
                                     ctypes.cast(descs, _P), cw, ch), fn)
        self._coded_n.append(len(descs))

    @property
    def ring_entries(self):
        return self.lib.jmh_coded_ring_entries(self.ctx)

    def pop_coded(self, cap=None):
        """The oldest pushed picture, a coded one: (bytes per slice, [(offset, nbytes, nbits, nbins)],
        {"ssd": (Y, U, V), "fallback": 0 / 1}).  cap: the size of the output buffer; a picture that
        needs more raises JmhError (status JMH_E_INVALID_ARG, .where filled) and stays poppable.
        Without cap the buffer grows to the picture's bytes and the pop is repeated."""
        if not getattr(self, "_coded_n", None):
            # no coded picture was pushed: let the library answer (JMH_E_STATE)
            w1, s1 = (JmhCodedBytes * 1)(), JmhCodedStats()
            _check(self.lib.jmh_frame_pop_coded(self.ctx, None, 0, ctypes.cast(w1, _P), ctypes.byref(s1)), "jmh_frame_pop_coded")
        n = self._coded_n[0]
        where, stats = (JmhCodedBytes * n)(), JmhCodedStats()
        size = cap if cap is not None else self.mbw * self.mbh * 64
        while True:
            out = np.zeros(max(size, 1), np.uint8)
            st = self.lib.jmh_frame_pop_coded(self.ctx, _ptr(out), size, ctypes.cast(where, _P), ctypes.byref(stats))
            total = where[n - 1].offset + where[n - 1].nbytes
            if st == JMH_E_INVALID_ARG and cap is None and total > size:
                size = total
                continue
            break
        wl = [(w.offset, w.nbytes, w.nbits, w.nbins) for w in where]
        if st != JMH_OK:
            e = JmhError(f"jmh_frame_pop_coded: {STATUS.get(st, st)} ({st})")
            e.status, e.where = st, wl
            raise e
        self._coded_n.pop(0)
        data = [out[w.offset:w.offset + w.nbytes].tobytes() for w in where]
        return data, wl, {"ssd": tuple(int(x) for x in stats.ssd), "fallback": int(stats.fallback)}

    # ---- pictures that are already on the device (include/jmhip_input.h) ----
    def device_alloc(self, nbytes):
        """jmh_device_malloc: a device address (int)."""
        p = ctypes.c_void_p()
        _check(self.lib.jmh_device_malloc(self.ctx, nbytes, ctypes.byref(p)), "jmh_device_malloc")
        return p.value

    def device_free(self, addr):
        _check(self.lib.jmh_device_free(self.ctx, _addr(addr)), "jmh_device_free")

    def device_stream(self):
        """jmh_device_stream_create: a stream handle (int) for DevicePicture.stream / device_upload."""
        p = ctypes.c_void_p()
        _check(self.lib.jmh_device_stream_create(self.ctx, ctypes.byref(p)), "jmh_device_stream_create")
        return p.value

    def device_stream_destroy(self, stream):
        _check(self.lib.jmh_device_stream_destroy(self.ctx, stream), "jmh_device_stream_destroy")

    def device_upload(self, dst, data, stream=None):
        """jmh_device_upload: the bytes of a numpy array to device address dst, queued on stream
        (None: done on return).  data is free on return either way."""
        data = np.ascontiguousarray(data)
        _check(self.lib.jmh_device_upload(self.ctx, _addr(dst), _ptr(data), data.nbytes, stream), "jmh_device_upload")

    # a device source is a DevicePicture or a DeviceTensor: its entry points end in "device" / "picture" or "tensor"
    def _upload_layout(self, layout, stream, base):
        if base is None:
            base = self.device_alloc(layout.buf.nbytes)
        self.device_upload(base, layout.buf, stream)
        src = layout.at(base, stream)
        src.base = base
        return src

    def _push_src(self, src, slice_type, qp, chroma_qp_offset, deblock):
        name = "jmh_frame_push_tensor" if isinstance(src, DeviceTensor) else "jmh_frame_push_device"
        fp = frame_params(slice_type, qp, chroma_qp_offset, deblock, self.cfg.rdo, self.cfg.bit_depth)
        s = src.struct()
        _check(getattr(self.lib, name)(self.ctx, ctypes.byref(s), ctypes.byref(fp)), name)

    def _push_coded_src(self, src, slice_type, qp, descs, crop, deblock, chroma_qp_offset, heads):
        name = "jmh_frame_push_coded_tensor" if isinstance(src, DeviceTensor) else "jmh_frame_push_coded_device"
        self._arm(heads)
        fp = frame_params(slice_type, qp, chroma_qp_offset, deblock, self.cfg.rdo, self.cfg.bit_depth)
        cw, ch = crop if crop is not None else (self.w, self.h)
        self._coded_n = getattr(self, "_coded_n", [])
        s = src.struct()
        _check(getattr(self.lib, name)(self.ctx, ctypes.byref(s), ctypes.byref(fp), len(descs), ctypes.cast(descs, _P), cw, ch), name)
        self._coded_n.append(len(descs))

    def _ingest_src(self, src):
        name = "jmh_ingest_tensor" if isinstance(src, DeviceTensor) else "jmh_ingest_picture"
        y = np.empty((self.h, self.w), self.pdt)
        u = np.empty((self.h // 2, self.w // 2), self.pdt)
        v = np.empty_like(u)
        s = src.struct()
        _check(getattr(self.lib, name)(self.ctx, ctypes.byref(s), _ptr(y), _ptr(u), _ptr(v), self.w, self.w // 2), name)
        return y, u, v

    def device_picture(self, layout, stream=None, base=None):
        """A HostLayout (to_device, to_device_rgb, to_device_yuv) uploaded: into base, or into a new allocation of exactly its
        bytes (the caller frees .base).  Returns the DevicePicture."""
        return self._upload_layout(layout, stream, base)

    def push_device(self, pic, slice_type, qp, chroma_qp_offset=0, deblock=None):
        """jmh_frame_push_device: push() of a DevicePicture; the library pads it to the coded size."""
        self._push_src(pic, slice_type, qp, chroma_qp_offset, deblock)

    def push_coded_device(self, pic, slice_type, qp, descs, crop=None, deblock=None, chroma_qp_offset=0, heads=None):
        """jmh_frame_push_coded_device: push_coded() of a DevicePicture."""
        self._push_coded_src(pic, slice_type, qp, descs, crop, deblock, chroma_qp_offset, heads)

    def ingest(self, pic):
        """jmh_ingest_picture, the unit seam: the DevicePicture packed and padded by the kernel, as
        (y, u, v) of the coded size."""
        return self._ingest_src(pic)

    # ---- device pushes scaled to a chosen size (include/jmhip_scale.h) ----
    def input_scale(self, out_w, out_h=None, filter=JMH_SCALE_LANCZOS3, chroma_left=False):
        """jmh_input_scale: from now on every device push and unit seam (pictures, RGB, tensors) takes a
        source of any even size up to JMH_SCALE_SRC_MAX, resamples it to out_w x out_h (even, at most
        the coded size) and pads that to the coded size.  input_scale(None) turns it off.  Pictures
        already pushed keep the setting of their push."""
        if out_w is None:
            _check(self.lib.jmh_input_scale(self.ctx, None), "jmh_input_scale")
            return
        s = JmhScale(filter, JMH_SCALE_CHROMA_LEFT if chroma_left else 0, out_w, out_h)
        _check(self.lib.jmh_input_scale(self.ctx, ctypes.byref(s)), "jmh_input_scale")

    def scale_info(self):
        """jmh_scale_info: the current setting as a dict, or None when it is off."""
        s, on = JmhScale(), ctypes.c_int(0)
        _check(self.lib.jmh_scale_info(self.ctx, ctypes.byref(s), ctypes.byref(on)), "jmh_scale_info")
        if not on.value:
            return None
        return {"filter": s.filter, "chroma_left": bool(s.flags & JMH_SCALE_CHROMA_LEFT), "out_width": s.out_width, "out_height": s.out_height}

    # ---- tensors that are already on the device (include/jmhip_tensor.h) ----
    def device_tensor(self, layout, stream=None, base=None):
        """A TensorLayout (to_device_tensor) uploaded: into base, or into a new allocation of exactly
        its bytes (the caller frees .base).  Returns the DeviceTensor."""
        return self._upload_layout(layout, stream, base)

    def from_torch(self, t, layout=None, order="rgb", flags=0, stream=None):
        """The DeviceTensor of a torch tensor on this context's device, with no copy: addresses from
        data_ptr(), strides from stride(), the element type from dtype (uint8, uint16, float16,
        bfloat16, float32).  layout "chw" or "hwc"; None infers it for a 3-D tensor whose first or
        last dimension is 3 or 4 (the last wins when both are).  Views are fine (permute, slices,
        crops) while the strides stay positive.  stream: the stream handle on which t is complete;
        None takes the stream torch is currently queueing on for t's device, and where that is the
        null stream, which cannot be ordered against, synchronises it.  Keep t alive, and do not
        write to it outside that stream, until input_wait() or the picture's pop.  torch must share
        this library's HIP runtime: import torch before the first Encoder is made."""
        import torch                                           # not at module load
        types = {torch.uint8: JMH_T_U8, torch.float16: JMH_T_F16, torch.bfloat16: JMH_T_BF16, torch.float32: JMH_T_F32}
        if hasattr(torch, "uint16"):
            types[torch.uint16] = JMH_T_U16
        if t.dtype not in types:
            raise ValueError(f"from_torch: no tensor dtype for {t.dtype}")
        if not t.is_cuda or t.dim() != 3:
            raise ValueError("from_torch takes a 3-D tensor on the device")
        _one_hip_runtime()
        if layout is None:
            layout = "hwc" if t.shape[2] in (3, 4) else "chw" if t.shape[0] in (3, 4) else None
        if layout not in ("chw", "hwc") or sorted(order) != ["b", "g", "r"]:
            raise ValueError("from_torch: layout is 'chw' or 'hwc' (not inferable from this shape) and order a permutation of 'rgb'")
        es = t.element_size()
        sc, sy, sx = (t.stride(i) * es for i in ((0, 1, 2) if layout == "chw" else (2, 0, 1)))
        h, w = (t.shape[1], t.shape[2]) if layout == "chw" else (t.shape[0], t.shape[1])
        if t.shape[0 if layout == "chw" else 2] < 3:
            raise ValueError("from_torch: fewer than three channels")
        if stream is None:
            cur = torch.cuda.current_stream(t.device)
            stream = cur.cuda_stream or None
            if stream is None:
                cur.synchronize()
        base = t.data_ptr()
        return DeviceTensor(types[t.dtype], flags, w, h, [base + order.index(c) * sc for c in "rgb"], sx, sy, stream)

    def push_tensor(self, t, slice_type, qp, chroma_qp_offset=0, deblock=None):
        """jmh_frame_push_tensor: push() of a DeviceTensor; the library quantises, converts and pads it."""
        self._push_src(t, slice_type, qp, chroma_qp_offset, deblock)

    def push_coded_tensor(self, t, slice_type, qp, descs, crop=None, deblock=None, chroma_qp_offset=0, heads=None):
        """jmh_frame_push_coded_tensor: push_coded() of a DeviceTensor."""
        self._push_coded_src(t, slice_type, qp, descs, crop, deblock, chroma_qp_offset, heads)

    def ingest_tensor(self, t):
        """jmh_ingest_tensor, the unit seam: the DeviceTensor quantised, converted, packed and padded
        by the kernel, as (y, u, v) of the coded size."""
        return self._ingest_src(t)

    # ---- decoded pictures pulled on the device (include/jmhip_output.h) ----
    def pull(self, dst, which=JMH_OUT_DEBLOCKED):
        """jmh_pull_picture: the current picture (the one the last pop returned), deblocked or
        JMH_OUT_RECON, cropped to dst's size and written into the planes of a DevicePictureOut, queued
        on dst.stream (None: complete on return)."""
        s = dst.struct()
        _check(self.lib.jmh_pull_picture(self.ctx, which, ctypes.byref(s)), "jmh_pull_picture")

    def pull_tensor(self, dst, which=JMH_OUT_DEBLOCKED):
        """jmh_pull_tensor: the same, converted to RGB and dequantised into a DeviceTensorOut."""
        s = dst.struct()
        _check(self.lib.jmh_pull_tensor(self.ctx, which, ctypes.byref(s)), "jmh_pull_tensor")

    def convert(self, y, u, v, dst):
        """jmh_convert_picture, the unit seam: host planes of the coded size through the pull's kernel
        into a DevicePictureOut; complete on return."""
        y, u, v = self._planes(y, u, v)
        s = dst.struct()
        _check(self.lib.jmh_convert_picture(self.ctx, _ptr(y), _ptr(u), _ptr(v), self.w, self.w // 2, ctypes.byref(s)), "jmh_convert_picture")

    def convert_tensor(self, y, u, v, dst):
        """jmh_convert_tensor, the unit seam: the same into a DeviceTensorOut."""
        y, u, v = self._planes(y, u, v)
        s = dst.struct()
        _check(self.lib.jmh_convert_tensor(self.ctx, _ptr(y), _ptr(u), _ptr(v), self.w, self.w // 2, ctypes.byref(s)), "jmh_convert_tensor")

    def device_out(self, layout, stream=None):
        """An OutLayout / OutTensorLayout (out_layout, out_tensor_layout) allocated: a new allocation of
        exactly its bytes (the caller frees .base).  Returns the DevicePictureOut / DeviceTensorOut."""
        base = self.device_alloc(layout.nbytes)
        d = layout.at(base, stream)
        d.base = base
        return d

    def output_wait(self):
        """jmh_device_output_wait: every pull queued so far has completed."""
        _check(self.lib.jmh_device_output_wait(self.ctx), "jmh_device_output_wait")

    def device_download(self, addr, nbytes, stream=None):
        """jmh_device_download: nbytes of device memory at addr as a uint8 array, copied behind the
        work queued on stream so far."""
        out = np.empty(nbytes, np.uint8)
        _check(self.lib.jmh_device_download(self.ctx, _ptr(out), _addr(addr), nbytes, stream), "jmh_device_download")
        return out

    def into_torch(self, t, order="rgb", flags=0, which=JMH_OUT_DEBLOCKED, layout=None):
        """The current picture pulled into a torch tensor on this context's device, with no copy: any
        (3, h, w) or (h, w, 3 or 4) tensor or view that from_torch would take, h x w being the crop.
        The pull is queued on the stream torch is currently queueing on for t's device, so torch work
        issued afterwards on that stream sees the picture; where that is the null stream, which cannot
        be ordered against, it is synchronised and the picture is complete on return."""
        d = self.from_torch(t, layout, order, flags)
        self.pull_tensor(DeviceTensorOut(d.dtype, d.flags, d.width, d.height, d.chans, d.stride_x, d.stride_y, d.stream), which)
        return t

    def to_torch(self, dtype, layout="chw", flags=0, size=None, which=JMH_OUT_DEBLOCKED, device=None):
        """into_torch of a new tensor: dtype a torch dtype (uint8, uint16, float16, bfloat16, float32),
        layout "chw" for (3, h, w) or "hwc" for (h, w, 3), size (width, height) of the crop, default the
        coded size."""
        import torch                                           # not at module load
        w, h = size if size is not None else (self.w, self.h)
        dev = device if device is not None else torch.device("cuda", torch.cuda.current_device())
        t = torch.empty((3, h, w) if layout == "chw" else (h, w, 3), dtype=dtype, device=dev)
        return self.into_torch(t, flags=flags, which=which, layout=layout)

    def input_wait(self):
        """jmh_device_input_wait: the last pushed device picture has been read; its planes are free."""
        _check(self.lib.jmh_device_input_wait(self.ctx), "jmh_device_input_wait")

    def input_clamped(self):
        """jmh_device_input_clamped: I010 samples above maxv in the picture last popped (or last ingest)."""
        n = ctypes.c_uint64()
        _check(self.lib.jmh_device_input_clamped(self.ctx, ctypes.byref(n)), "jmh_device_input_clamped")
        return n.value

    def pop_into(self, y, u, v):
        """What lencod does per picture: jmh_frame_pop, the results in place (a zero-copy view of the
        library's host array, valid until the next pop) and the deblocked picture (the recon file /
        PSNR input) into the caller's planes.  Returns the results view."""
        _check(self.lib.jmh_frame_pop(self.ctx), "jmh_frame_pop")
        fn = "jmh_read_deblocked" + self.sfx
        _check(getattr(self.lib, fn)(self.ctx, _ptr(y), _ptr(u), _ptr(v), self.w, self.w // 2), fn)
        return self.results_view()

    def results_view(self):
        n = self.mbw * self.mbh
        p = self.lib.jmh_get_mb_result(self.ctx, 0)
        if not p:
            raise JmhError("no results")
        buf = (ctypes.c_char * (n * MB_RESULT_DTYPE.itemsize)).from_address(p)
        return np.frombuffer(buf, dtype=MB_RESULT_DTYPE)

    @property
    def depth(self):
        return self.lib.jmh_pipeline_depth(self.ctx)

    def results(self):
        n = self.mbw * self.mbh
        p = self.lib.jmh_get_mb_result(self.ctx, 0)
        if not p:
            raise JmhError("no results")
        buf = (ctypes.c_char * (n * MB_RESULT_DTYPE.itemsize)).from_address(p)
        return np.frombuffer(bytes(buf), dtype=MB_RESULT_DTYPE).copy()

    def _read(self, fn):
        fn += self.sfx
        y = np.empty((self.h, self.w), self.pdt)
        u = np.empty((self.h // 2, self.w // 2), self.pdt)
        v = np.empty_like(u)
        _check(getattr(self.lib, fn)(self.ctx, _ptr(y), _ptr(u), _ptr(v), self.w, self.w // 2), fn)
        return y, u, v

    def recon(self):
        return self._read("jmh_read_recon")

    def deblocked(self):
        """DeblockFrame output of the last encode(..., deblock=...) (jmh_read_deblocked)."""
        return self._read("jmh_read_deblocked")

    # ---- device-resident path (bench) ----
    def load_frame(self, slot, y, u, v):
        y, u, v = self._planes(y, u, v)
        fn = "jmh_load_frame" + self.sfx
        _check(getattr(self.lib, fn)(self.ctx, slot, _ptr(y), _ptr(u), _ptr(v), self.w, self.w // 2), fn)

    def set_reference_slot(self, slot):
        _check(self.lib.jmh_set_reference_slot(self.ctx, slot), "jmh_set_reference_slot")

    def encode_slot(self, slot, slice_type, qp, deblock=None):
        fp = frame_params(slice_type, qp, deblock=deblock, rdo=self.cfg.rdo, bit_depth=self.cfg.bit_depth)
        _check(self.lib.jmh_encode_slot(self.ctx, slot, ctypes.byref(fp)), "jmh_encode_slot")

    def sync(self):
        """Drain: every picture in flight runs to completion (jmh_sync)."""
        _check(self.lib.jmh_sync(self.ctx), "jmh_sync")

    def wait_issued(self):
        """Wait for the launches issued so far; pictures in flight stay in flight (jmh_wait_issued)."""
        _check(self.lib.jmh_wait_issued(self.ctx), "jmh_wait_issued")

    def timing(self):
        """Event sums since the previous call (waits for the issued launches, does not drain)."""
        t = JmhTiming()
        _check(self.lib.jmh_get_timing(self.ctx, ctypes.byref(t)), "jmh_get_timing")
        return t

    # ---- CAVLC slice data on the device (jmh_cavlc_write_slices / _results) ----
    def _cavlc(self, call, what, descs, cap, with_where):
        n = len(descs)
        if cap is None:          # the documented bound: no picture needs more
            cap = self.mbw * self.mbh * (JMW_MB_MAX_BITS // 8) + 2 * n
        out = np.zeros(max(cap, 1), np.uint8)
        where = (JmhSliceBytes * n)()
        _check(call(n, ctypes.cast(descs, _P), _ptr(out), cap, ctypes.cast(where, _P)), what)
        data = [out[w.offset:w.offset + w.nbytes].tobytes() for w in where]
        return (data, [(w.offset, w.nbytes, w.nbits) for w in where]) if with_where else data

    def cavlc_slices(self, descs, cap=None, with_where=False):
        """slice_data() + rbsp_trailing_bits of every slice (a JmhSliceDesc array, see slice_descs) of
        the picture last popped / waited for, written on the device: a list of bytes, one per slice
        (behind each slice header's whole bytes they are the slice's RBSP)."""
        return self._cavlc(lambda *a: self.lib.jmh_cavlc_write_slices(self.ctx, *a), "jmh_cavlc_write_slices", descs, cap, with_where)

    def cavlc_results(self, res, descs, cap=None, with_where=False):
        """The same for caller-supplied results (MB_RESULT_DTYPE[mbw * mbh]); no picture needed."""
        res = np.ascontiguousarray(res, MB_RESULT_DTYPE)
        if res.size != self.mbw * self.mbh:
            raise JmhError(f"cavlc_results: {res.size} results for {self.mbw * self.mbh} macroblocks")
        return self._cavlc(lambda *a: self.lib.jmh_cavlc_write_results(self.ctx, _ptr(res), *a), "jmh_cavlc_write_results", descs, cap,
                           with_where)

    # ---- CABAC slice data on the device (jmh_cabac_write_slices / _results) ----
    def _cabac(self, call, what, descs, cap, with_where):
        n = len(descs)
        if cap is None:          # the documented bound: no picture needs more
            cap = cabac_max_bytes(self.mbw * self.mbh, n)
        out = np.zeros(max(cap, 1), np.uint8)
        where = (JmhCabacSliceBytes * n)()
        _check(call(n, ctypes.cast(descs, _P), _ptr(out), cap, ctypes.cast(where, _P)), what)
        data = [out[w.offset:w.offset + w.nbytes].tobytes() for w in where]
        return (data, [(w.offset, w.nbytes, w.nbins) for w in where]) if with_where else data

    def cabac_slices(self, descs, cap=None, with_where=False):
        """The CABAC slice_data() up to the rbsp_stop_one_bit of every slice (a JmhCabacSliceDesc array,
        see cabac_slice_descs) of the picture last popped / waited for, written on the device: a list of
        bytes, one per slice (behind each slice header and its cabac_alignment_one_bits they are the
        slice's RBSP).  with_where: also (offset, nbytes, nbins) per slice."""
        return self._cabac(lambda *a: self.lib.jmh_cabac_write_slices(self.ctx, *a), "jmh_cabac_write_slices", descs, cap, with_where)

    def cabac_results(self, res, descs, cap=None, with_where=False):
        """The same for caller-supplied results (MB_RESULT_DTYPE[mbw * mbh]); no picture needed."""
        res = np.ascontiguousarray(res, MB_RESULT_DTYPE)
        if res.size != self.mbw * self.mbh:
            raise JmhError(f"cabac_results: {res.size} results for {self.mbw * self.mbh} macroblocks")
        return self._cabac(lambda *a: self.lib.jmh_cabac_write_results(self.ctx, _ptr(res), *a), "jmh_cabac_write_results", descs, cap,
                           with_where)

    def cabac_split(self, chunk_bins):
        """jmh_cabac_set_split: the CABAC writer (cabac_slices, cabac_results, coded pictures pushed from
        now on) cuts every slice into chunks of chunk_bins bins (16..65536) and codes all of them at
        once; 0 (the state of a new encoder): one wave per slice.  The bytes are the same."""
        _check(self.lib.jmh_cabac_set_split(self.ctx, int(chunk_bins)), "jmh_cabac_set_split")

    def cabac_split_info(self):
        """jmh_cabac_split_stats of the last cabac_slices / cabac_results call: a dict of chunk_bins (0:
        it ran unsplit), chunks, longest_slice_chunks, scratch_bytes; and the current setting."""
        info = JmhCabacSplitInfo()
        _check(self.lib.jmh_cabac_split_stats(self.ctx, ctypes.byref(info)), "jmh_cabac_split_stats")
        return dict(chunk_bins=info.chunk_bins, chunks=info.chunks, longest_slice_chunks=info.longest_slice_chunks,
                    scratch_bytes=info.scratch_bytes, setting=self.lib.jmh_cabac_get_split(self.ctx))

    # ---- unit seams ----
    def spiral_positions(self, search_range):
        """jmh_spiral_positions (include/jmhip_spiral.h): the kernels' spiral decode on the device, as
        an int32 array [(2 sr + 1)^2][2] of (x, y) by spiral index."""
        fn = self.lib.jmh_spiral_positions
        fn.restype, fn.argtypes = _SIGS_SPIRAL["jmh_spiral_positions"]
        side = 2 * search_range + 1
        out = np.empty((side * side, 2), np.int32)
        _check(fn(self.ctx, search_range, _ptr(out)), "jmh_spiral_positions")
        return out

    def sad_table(self, mb_xy, centres):
        mb_xy = np.ascontiguousarray(mb_xy, np.int32)
        centres = np.ascontiguousarray(centres, np.int32)
        n = mb_xy.shape[0]
        side = 2 * self.cfg.search_range + 1
        out = np.empty((n, 16, side * side), np.uint16)
        _check(self.lib.jmh_ffs_sad_table(self.ctx, n, _ptr(mb_xy), _ptr(centres), _ptr(out)),
               "jmh_ffs_sad_table")
        return out

    def tq4x4(self, resid, pred, qp, intra):
        resid = np.ascontiguousarray(resid, np.int16)
        pred = np.ascontiguousarray(pred, np.uint8)
        n = resid.shape[0]
        lev = np.empty((n, 16), np.int16)
        rec = np.empty((n, 16), np.uint8)
        cc = np.empty(n, np.int32)
        nz = np.empty(n, np.int32)
        _check(self.lib.jmh_tq4x4_batch(self.ctx, n, _ptr(resid), _ptr(pred), qp, intra, _ptr(lev),
                                        _ptr(rec), _ptr(cc), _ptr(nz)), "jmh_tq4x4_batch")
        return lev, rec, cc, nz

    def tq8x8(self, resid, pred, qp, intra):
        resid = np.ascontiguousarray(resid, np.int16)
        pred = np.ascontiguousarray(pred, np.uint8)
        n = resid.shape[0]
        lev = np.empty((n, 64), np.int16)
        rec = np.empty((n, 64), np.uint8)
        cc = np.empty(n, np.int32)
        nz = np.empty(n, np.int32)
        _check(self.lib.jmh_tq8x8_batch(self.ctx, n, _ptr(resid), _ptr(pred), qp, intra, _ptr(lev),
                                        _ptr(rec), _ptr(cc), _ptr(nz)), "jmh_tq8x8_batch")
        return lev, rec, cc, nz

    def read_qpel(self):
        out = np.empty((16, self.h + 8, self.w + 8), np.uint8)
        _check(self.lib.jmh_read_qpel(self.ctx, _ptr(out)), "jmh_read_qpel")
        return out

    def search_pictures(self, cur_y, ref_y):
        cur_y, ref_y = np.ascontiguousarray(cur_y, np.uint8), np.ascontiguousarray(ref_y, np.uint8)
        _check(self.lib.jmh_search_pictures(self.ctx, _ptr(cur_y), _ptr(ref_y), self.w), "jmh_search_pictures")

    def block_motion_search(self, reqs):
        """reqs: a ctypes array of JmhBlockSearch; returns the JmhBlockResult array."""
        out = (JmhBlockResult * len(reqs))()
        _check(self.lib.jmh_block_motion_search(self.ctx, len(reqs), ctypes.cast(reqs, _P), ctypes.cast(out, _P)),
               "jmh_block_motion_search")
        return out

    # ---- High 10 seams (16-bit samples, bit_depth 8..10) ----
    def search_pictures_u16(self, cur_y, ref_y, bit_depth):
        cur_y, ref_y = np.ascontiguousarray(cur_y, np.uint16), np.ascontiguousarray(ref_y, np.uint16)
        _check(self.lib.jmh_search_pictures_u16(self.ctx, _ptr(cur_y), _ptr(ref_y), self.w, bit_depth),
               "jmh_search_pictures_u16")

    def block_motion_search_u16(self, reqs):
        out = (JmhBlockResult * len(reqs))()
        _check(self.lib.jmh_block_motion_search_u16(self.ctx, len(reqs), ctypes.cast(reqs, _P), ctypes.cast(out, _P)),
               "jmh_block_motion_search_u16")
        return out

    def sad_table_u16(self, mb_xy, centres):
        mb_xy = np.ascontiguousarray(mb_xy, np.int32)
        centres = np.ascontiguousarray(centres, np.int32)
        n = mb_xy.shape[0]
        side = 2 * self.cfg.search_range + 1
        out = np.empty((n, 16, side * side), np.uint16)
        _check(self.lib.jmh_ffs_sad_table_u16(self.ctx, n, _ptr(mb_xy), _ptr(centres), _ptr(out)), "jmh_ffs_sad_table_u16")
        return out

    def tq_u16(self, resid, pred, qp, intra, bit_depth):
        """dct_luma (resid[n][16]) or dct_luma8x8 (resid[n][64]) on 16-bit samples."""
        resid = np.ascontiguousarray(resid, np.int16)
        pred = np.ascontiguousarray(pred, np.uint16)
        n, el = resid.shape
        lev = np.empty((n, el), np.int16)
        rec = np.empty((n, el), np.uint16)
        cc = np.empty(n, np.int32)
        nz = np.empty(n, np.int32)
        fn = self.lib.jmh_tq4x4_batch_u16 if el == 16 else self.lib.jmh_tq8x8_batch_u16
        _check(fn(self.ctx, n, _ptr(resid), _ptr(pred), qp, intra, bit_depth, _ptr(lev), _ptr(rec), _ptr(cc), _ptr(nz)),
               "jmh_tq%s_batch_u16" % ("4x4" if el == 16 else "8x8"))
        return lev, rec, cc, nz


# ---- synthetic source (product host plumbing, libjmhost.so) ------------------------------
_host = None


def load_host(path=HOST_LIB_PATH):
    global _host
    if _host is None:
        if not os.path.exists(path):
            raise JmhError(f"libjmhost.so not found at {path}: build it with __graft_entry__.build()")
        _host = ctypes.CDLL(path)
        _host.jm_synth_frame.restype = None
        _host.jm_synth_frame.argtypes = [_P, _I, _I, ctypes.c_uint64, _I]
    return _host


def cavlc_ref(width, height, transform_8x8_mode, constrained_intra, res, descs, with_where=False):
    """The host writer (host/bitstream.c through host/cavlc_ref.c) behind the arguments of
    Encoder.cavlc_results: the reference of the device writer.  A list of bytes, one per slice."""
    host = load_host()
    host.jm_cavlc_ref.restype = _I
    host.jm_cavlc_ref.argtypes = [_I, _I, _I, _I, _P, _I, _P, _P, ctypes.c_size_t, _P]
    res = np.ascontiguousarray(res, MB_RESULT_DTYPE)
    n = len(descs)
    cap = res.size * (JMW_MB_MAX_BITS // 8) + 2 * n
    out = np.zeros(cap, np.uint8)
    where = (JmhSliceBytes * n)()
    _check(host.jm_cavlc_ref(width, height, transform_8x8_mode, constrained_intra, _ptr(res), n, ctypes.cast(descs, _P), _ptr(out), cap,
                             ctypes.cast(where, _P)), "jm_cavlc_ref")
    data = [out[w.offset:w.offset + w.nbytes].tobytes() for w in where]
    return (data, [(w.offset, w.nbytes, w.nbits) for w in where]) if with_where else data


def cabac_ref(width, height, transform_8x8_mode, constrained_intra, res, descs, with_where=False, cap=None):
    """The host CABAC writer (host/cabac.c through host/cabac_ref.c) behind the arguments of
    Encoder.cabac_results: the reference of the device writer.  A list of bytes, one per slice;
    with_where: also (offset, nbytes, nbins) per slice."""
    host = load_host()
    host.jm_cabac_ref.restype = _I
    host.jm_cabac_ref.argtypes = [_I, _I, _I, _I, _P, _I, _P, _P, ctypes.c_size_t, _P]
    res = np.ascontiguousarray(res, MB_RESULT_DTYPE)
    n = len(descs)
    if cap is None:
        cap = cabac_max_bytes(res.size, n)
    out = np.zeros(max(cap, 1), np.uint8)
    where = (JmhCabacSliceBytes * n)()
    _check(host.jm_cabac_ref(width, height, transform_8x8_mode, constrained_intra, _ptr(res), n, ctypes.cast(descs, _P), _ptr(out), cap,
                             ctypes.cast(where, _P)), "jm_cabac_ref")
    data = [out[w.offset:w.offset + w.nbytes].tobytes() for w in where]
    return (data, [(w.offset, w.nbytes, w.nbins) for w in where]) if with_where else data


def deblock_ref(rec_yuv, results, mbw, mbh, qp, chroma_qp_offset=0, alpha_div2=0, beta_div2=0, bit_depth=8):
    """The host deblocker (host/deblock.c through host/deblock_ref.c) on a reconstructed picture
    (y, u, v) and its results (MB_RESULT_DTYPE[mbw * mbh]), disable_deblocking_filter_idc 0:
    the filtered (y, u, v), new arrays."""
    host = load_host()
    host.jm_deblock_ref.restype = _I
    host.jm_deblock_ref.argtypes = [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I]
    res = np.ascontiguousarray(results, MB_RESULT_DTYPE)
    if res.size != mbw * mbh:
        raise JmhError(f"deblock_ref: {res.size} results for {mbw * mbh} macroblocks")
    y, u, v = (np.array(p, np.uint16 if bit_depth > 8 else np.uint8, order="C") for p in rec_yuv)
    if y.shape != (16 * mbh, 16 * mbw) or u.shape != (8 * mbh, 8 * mbw) or v.shape != u.shape:
        raise JmhError(f"deblock_ref: planes {y.shape} {u.shape} {v.shape} for {mbw} x {mbh} macroblocks")
    _check(host.jm_deblock_ref(_ptr(y), _ptr(u), _ptr(v), _ptr(res), mbw, mbh, qp, chroma_qp_offset, alpha_div2, beta_div2, bit_depth),
           "jm_deblock_ref")
    return y, u, v


class _JmPic(ctypes.Structure):
    _fields_ = [("w", ctypes.c_int), ("h", ctypes.c_int), ("y", _P), ("u", _P), ("v", _P),
                ("bd", ctypes.c_int), ("Y", _P), ("U", _P), ("V", _P)]


def synth_frame(disp_w, disp_h, seed, index, bit_depth=8):
    """Deterministic synthetic 4:2:0 picture (coded size = multiple of 16), as (y, u, v); bit_depth
    9 / 10: 16-bit samples (jm_synth_frame_hbd)."""
    host = load_host()
    if bit_depth > 8:
        cw, ch = (disp_w + 15) // 16 * 16, (disp_h + 15) // 16 * 16
        y = np.zeros((ch, cw), np.uint16)
        u = np.zeros((ch // 2, cw // 2), np.uint16)
        v = np.zeros_like(u)
        host.jm_synth_frame_hbd.restype = None
        host.jm_synth_frame_hbd.argtypes = [_P, _P, _P, _I, _I, _I, _I, ctypes.c_uint64, _I, _I]
        host.jm_synth_frame_hbd(_ptr(y), _ptr(u), _ptr(v), cw, ch, disp_w, disp_h, seed, index, bit_depth)
        return y, u, v
    cw, ch = (disp_w + 15) // 16 * 16, (disp_h + 15) // 16 * 16
    y = np.zeros((ch, cw), np.uint8)
    u = np.zeros((ch // 2, cw // 2), np.uint8)
    v = np.zeros_like(u)
    pic = _JmPic(cw, ch, y.ctypes.data, u.ctypes.data, v.ctypes.data, 8, None, None, None)
    host.jm_synth_frame(ctypes.byref(pic), disp_w, disp_h, seed, index)
    return y, u, v
