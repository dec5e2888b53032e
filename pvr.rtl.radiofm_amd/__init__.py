"""pvr.rtl.radiofm_amd -- MI355X-native FM broadcast decoder (hot path of pvr.rtl.radiofm).

The product is the C-ABI shared library ``libfmd_hip.so`` (include/fmd.h) built from csrc/.
This module is only the ctypes plumbing the tests and bench.py use to reach it; the directory
name contains dots, so load it through ``__graft_entry__.load_package()`` (importlib).

There is no CPU fallback here: if the HIP library is missing or no GPU is usable, the calls
raise.  Nothing in this package imports or links oracle/.
"""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libfmd_hip.so")
_LIB = None

FMD_MAX_BLOCK = 65536
FMD_MIN_BLOCK = 8192
FMD_WARN_RDS_LOST = 1
# IQ input formats (include/fmd.h FMD_IQ_*): the `format` argument of the _fmt entry points
FMD_IQ_F32, FMD_IQ_U8, FMD_IQ_S8, FMD_IQ_S16 = 0, 1, 2, 3
IQ_BYTES = {FMD_IQ_F32: 8, FMD_IQ_U8: 2, FMD_IQ_S8: 2, FMD_IQ_S16: 4}  # per IQ sample
FMD_REAL_F32, FMD_REAL_S8, FMD_REAL_S16 = 16, 18, 19  # real samples, a real band splitter's input only (split.py)
# audio output formats (include/fmd.h FMD_PCM_*): the `pcm_format` argument of the _pcm entry points
FMD_PCM_F32, FMD_PCM_S16 = 0, 1
PCM_BYTES = {FMD_PCM_F32: 4, FMD_PCM_S16: 2}  # per audio sample
# multiplex output formats (include/fmd.h FMD_MPX_*): the `mpx_format` argument of the _mpx entry points
FMD_MPX_F32, FMD_MPX_S16 = 0, 1
MPX_BYTES = {FMD_MPX_F32: 4, FMD_MPX_S16: 2}  # per multiplex sample
# mono feed formats (include/fmd.h FMD_FEED_*): the `feed_format` argument of the _feed entry points
FMD_FEED_F32, FMD_FEED_S16 = 0, 1
FEED_BYTES = {FMD_FEED_F32: 4, FMD_FEED_S16: 2}  # per feed sample
# channel IQ formats (include/fmd.h FMD_CIQ_*): the `ciq.format` of a call record
FMD_CIQ_F32, FMD_CIQ_S16 = 0, 1
CIQ_BYTES = {FMD_CIQ_F32: 8, FMD_CIQ_S16: 4}  # per complex sample
# channel IQ rows as a call's INPUT (include/fmd.h FMD_IN_CIQ_*): two more values of a call record's iq_format
FMD_IN_CIQ_F32, FMD_IN_CIQ_S16 = 32, 33
IN_CIQ_BYTES = {FMD_IN_CIQ_F32: 8, FMD_IN_CIQ_S16: 4}  # per complex sample

TAPS = {"demod": 0, "baseband": 1, "pilot38": 2, "mono_rs": 3, "stereo_rs": 4, "rds_lpf": 5,
        "rds_pll": 6, "rds_mf": 7, "rds_sync": 8}
DESIGN = {"if_taps": 0, "rs_taps": 1, "audio_lpf": 2, "rds_lpf": 3, "rds_mf": 4, "scalars": 5,
          "lut0": 6}
SCALAR_NAMES = [
    "tuning_shift", "demod_gain", "de_alpha", "pll_alpha", "pll_beta", "nco_hl", "nco_ll",
    "pilot_minfreq", "pilot_maxfreq", "pilot_b0", "pilot_a1", "pilot_a2", "pilot_lf_b0",
    "pilot_lf_b1", "pilot_freq", "pilot_lock_delay", "resamp_order", "resamp_step",
    "rds_rate", "rds_nco_inc", "rds_osc_cos", "rds_osc_sin", "rds_pll_alpha", "rds_pll_beta",
    "rds_nco_hl", "rds_nco_ll", "fs_bb", "rds_mf_len",
    "notch_b0", "notch_b1", "notch_b2", "notch_a1", "notch_a2",
    "bitsync_b0", "bitsync_b1", "bitsync_b2", "bitsync_a1", "bitsync_a2",
]


class FmdParams(C.Structure):
    _fields_ = [
        ("sample_rate_if", C.c_double),
        ("tuning_offset", C.c_double),
        ("sample_rate_pcm", C.c_double),
        ("bandwidth_pcm", C.c_double),
        ("downsample", C.c_uint),
        ("us_version", C.c_int),
        ("table_size", C.c_uint),
        ("if_filter_order", C.c_uint),
        ("fir_reduction", C.c_int),
    ]


UECP_CB = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_uint, C.POINTER(C.c_uint8), C.c_uint)
NAME_CB = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_uint, C.c_char_p)
ACTIVE_CB = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_uint)


class FmdCallbacks(C.Structure):
    _fields_ = [("add_uecp_frame", UECP_CB), ("set_channel_name", NAME_CB),
                ("is_setting_active", ACTIVE_CB)]


class FmdStatus(C.Structure):
    _fields_ = [
        ("stereo_detected", C.c_int),
        ("tuning_offset", C.c_float),
        ("interface_level", C.c_float),
        ("baseband_level", C.c_float),
        ("pilot_level", C.c_float),
        ("rds_state", C.c_int),
    ]


class FmdRdsGroup(C.Structure):
    _fields_ = [("channel", C.c_uint32), ("call_index", C.c_uint32), ("blocks", C.c_uint16 * 4)]


RDS_GROUP_DTYPE = np.dtype([("channel", "<u4"), ("call_index", "<u4"), ("blocks", "<u2", (4,))])
assert RDS_GROUP_DTYPE.itemsize == C.sizeof(FmdRdsGroup)


class FmdRdsBlock(C.Structure):
    _fields_ = [("channel", C.c_uint32), ("call_index", C.c_uint32), ("bit_index", C.c_uint32), ("raw", C.c_uint32),
                ("word", C.c_uint16), ("sample", C.c_uint16), ("position", C.c_uint8), ("status", C.c_uint8),
                ("state", C.c_uint8), ("corrected", C.c_uint8)]


class FmdRdsQuality(C.Structure):
    _fields_ = [(f, C.c_uint32) for f in ("bits", "candidates", "blocks", "corrected", "failed", "sync_acquired",
                                          "sync_lost", "groups")]


RDS_BLOCK_DTYPE = np.dtype([("channel", "<u4"), ("call_index", "<u4"), ("bit_index", "<u4"), ("raw", "<u4"),
                            ("word", "<u2"), ("sample", "<u2"), ("position", "u1"), ("status", "u1"), ("state", "u1"),
                            ("corrected", "u1")])
RDS_QUALITY_DTYPE = np.dtype([(f, "<u4") for f, _ in FmdRdsQuality._fields_])
assert C.sizeof(FmdRdsBlock) == 24 and RDS_BLOCK_DTYPE.itemsize == 24
assert C.sizeof(FmdRdsQuality) == 32 and RDS_QUALITY_DTYPE.itemsize == 32
# block observation modes (include/fmd.h FMD_RDS_BLOCKS_*)
FMD_RDS_BLOCKS_OFF, FMD_RDS_BLOCKS_COUNT, FMD_RDS_BLOCKS_RECORD = 0, 1, 2
# a loudness block record (include/fmd.h fmd_loud_block)
LOUD_BLOCK_DTYPE = np.dtype([("z_l", "<f4"), ("z_r", "<f4"), ("peak_l", "<f4"), ("peak_r", "<f4")])
assert LOUD_BLOCK_DTYPE.itemsize == 16

class FmdAudioLevel(C.Structure):
    _fields_ = [("mean", C.c_float), ("rms", C.c_float), ("level", C.c_float)]


class FmdDemuxPacket(C.Structure):
    _fields_ = [("stream_id", C.c_int), ("size", C.c_int), ("pts", C.c_double),
                ("duration", C.c_double), ("data", C.POINTER(C.c_uint8))]


class FmdPvrSignalStatus(C.Structure):
    _fields_ = [("adapter_name", C.c_char * 128), ("adapter_status", C.c_char * 256),
                ("provider_name", C.c_char * 64), ("signal", C.c_int), ("snr", C.c_int)]


class FmdScanParams(C.Structure):
    _fields_ = [("sample_rate_if", C.c_double), ("table_size", C.c_uint), ("nfft", C.c_uint),
                ("half_width_hz", C.c_double), ("min_separation_hz", C.c_double), ("threshold_db", C.c_float),
                ("floor_quantile", C.c_float)]


class FmdSplitParams(C.Structure):
    """fmd_split_params (include/fmd.h): 0 = the field's default."""
    _fields_ = [("sample_rate_in", C.c_double), ("decimation", C.c_uint), ("filter_order", C.c_uint),
                ("cutoff", C.c_double), ("table_size", C.c_uint), ("out_scale", C.c_float)]


class FmdChanParams(C.Structure):
    """fmd_chan_params (include/fmd.h): 0 = the field's default (n_bins and decimation have none)."""
    _fields_ = [("sample_rate_in", C.c_double), ("n_bins", C.c_uint), ("decimation", C.c_uint),
                ("filter_order", C.c_uint), ("cutoff", C.c_double), ("out_scale", C.c_float)]


class FmdScanCandidate(C.Structure):
    _fields_ = [("shift", C.c_int32), ("offset_hz", C.c_float), ("power_db", C.c_float), ("snr_db", C.c_float)]


SCAN_CANDIDATE_DTYPE = np.dtype([("shift", "<i4"), ("offset_hz", "<f4"), ("power_db", "<f4"), ("snr_db", "<f4")])
assert SCAN_CANDIDATE_DTYPE.itemsize == C.sizeof(FmdScanCandidate)


class FmdRows(C.Structure):
    """fmd_rows: one output of a call record; p None: not delivered."""
    _fields_ = [("p", C.c_void_p), ("format", C.c_int), ("stride", C.c_size_t), ("count", C.POINTER(C.c_uint))]


class FmdCall(C.Structure):
    """fmd_call: a process call as one record (the _call entry points)."""
    _fields_ = [("size", C.c_size_t), ("iq", C.c_void_p), ("iq_format", C.c_int), ("iq_channel_stride", C.c_size_t),
                ("samples", C.c_uint), ("audio", FmdRows), ("mpx", FmdRows), ("feed", FmdRows), ("ciq", FmdRows),
                ("stream", C.c_void_p)]


def make_rows(p=None, fmt=0, stride=0, count=None):
    """An FmdRows; count: a ctypes c_uint that takes the elements per row the call wrote."""
    return FmdRows(p, int(fmt), int(stride), C.pointer(count) if count is not None else None)


def ciq_in_of(rows):
    """(pointer, FMD_IN_CIQ_* format, stride in complex samples, M) of channel IQ rows given as a call's input: a torch
    tensor or numpy array of complex64 [C, M] / [M] (FMD_IN_CIQ_F32) or int16 [C, M, 2] / [M, 2] (re, im;
    FMD_IN_CIQ_S16), the samples of a row contiguous.  The format is the dtype's; any other dtype or layout raises:
    nothing is converted or copied silently."""
    name = str(rows.dtype).replace("torch.", "")
    fmt = {"complex64": FMD_IN_CIQ_F32, "int16": FMD_IN_CIQ_S16}.get(name)
    if fmt is None:
        raise FmdError(FMD_ERR_ARG_TEXT % ("no channel IQ input format for dtype %s (complex64, int16)" % name))
    shape = tuple(int(v) for v in rows.shape)
    nd = len(shape) - (1 if fmt == FMD_IN_CIQ_S16 else 0)
    if nd not in (1, 2) or (fmt == FMD_IN_CIQ_S16 and shape[-1] != 2):
        raise FmdError(FMD_ERR_ARG_TEXT % "channel IQ input rows are complex64 [C, M] or int16 [C, M, 2]")
    if hasattr(rows, "data_ptr"):  # torch: strides in elements
        ptr, strides = rows.data_ptr(), tuple(int(v) for v in rows.stride())
    else:
        ptr, strides = rows.ctypes.data, tuple(int(v) // rows.dtype.itemsize for v in rows.strides)
    per = 2 if fmt == FMD_IN_CIQ_S16 else 1  # array elements per complex sample
    if (fmt == FMD_IN_CIQ_S16 and strides[-1] != 1) or strides[nd - 1] != per or (nd == 2 and strides[0] % per):
        raise FmdError(FMD_ERR_ARG_TEXT % "the samples of a channel IQ input row must be contiguous")
    return ptr, fmt, (strides[0] // per if nd == 2 else 0), shape[nd - 1]


def make_call(iq=None, iq_format=None, iq_stride=None, samples=None, audio=None, mpx=None, feed=None, ciq=None,
              stream=None, ciq_in=None):
    """An FmdCall with its size filled in; audio / mpx / feed / ciq: FmdRows or None.
    ciq_in: channel IQ rows as the call's input (ciq_in_of: complex64 or int16 by dtype) in place of iq / iq_format /
    iq_stride / samples -- a stride or a length given beside it wins.  The caller keeps the rows alive."""
    if ciq_in is not None:
        if iq is not None or iq_format is not None:
            raise FmdError(FMD_ERR_ARG_TEXT % "a call takes iq or ciq_in, not both")
        iq, iq_format, stride, m = ciq_in_of(ciq_in)
        iq_stride = stride if iq_stride is None else iq_stride
        samples = m if samples is None else samples
    call = FmdCall(size=C.sizeof(FmdCall), iq=iq, iq_format=int(iq_format), iq_channel_stride=int(iq_stride),
                   samples=int(samples), stream=stream)
    for name, rows in (("audio", audio), ("mpx", mpx), ("feed", feed), ("ciq", ciq)):
        if rows is not None:
            setattr(call, name, rows)
    return call


STREAM_AUDIO, STREAM_RDS, STREAM_CHANGE, STREAM_TIME_BASE = 1, 2, -11, 1000000

EXPORTS = [
    "fmd_debug_math", "fmd_batch_debug_serial_probe", "fmd_design_lanczos", "fmd_design_lp_kaiser", "fmd_design_biquad", "fmd_design_tuner_lut",
    "fmd_batch_get_audio_level", "fmd_receiver_open", "fmd_receiver_close", "fmd_receiver_write_iq",
    "fmd_receiver_write_u8", "fmd_receiver_end", "fmd_receiver_queued_samples",
    "fmd_receiver_set_stream_change", "fmd_receiver_demux_read", "fmd_receiver_signal_status",
    "fmd_receiver_pvr_signal_status", "fmd_receiver_decoder",
    "fmd_create", "fmd_destroy", "fmd_reset", "fmd_process_stream", "fmd_process_stream_u8",
    "fmd_get_status", "fmd_batch_process_device_u8", "fmd_batch_process_host_u8",
    "fmd_batch_create", "fmd_batch_destroy", "fmd_batch_reset", "fmd_batch_channels",
    "fmd_batch_min_samples",
    "fmd_batch_max_audio_floats", "fmd_batch_process_device", "fmd_batch_process_host",
    "fmd_batch_collect_rds", "fmd_batch_collect_rds_lagged", "fmd_batch_export_rds_device",
    "fmd_batch_set_concurrency", "fmd_batch_set_channels_per_capture", "fmd_batch_streams_sharing_queue",
    "fmd_batch_wait", "fmd_batch_wait_lagged", "fmd_batch_get_status", "fmd_batch_get_tap", "fmd_batch_get_design",
    "fmd_batch_set_debug_taps", "fmd_batch_set_profiling", "fmd_batch_get_stage_ms", "fmd_stage_name", "fmd_last_error",
    "fmd_version", "fmd_group_decoder_create", "fmd_group_decoder_destroy",
    "fmd_group_decoder_reset", "fmd_group_decoder_push", "fmd_uecp_stuff_frame",
    "fmd_batch_take_rds_lost", "fmd_batch_status_call_index",
    "fmd_batch_debug_set_spin_limit", "fmd_batch_debug_timeline", "fmd_batch_debug_set",
    "fmd_batch_debug_stream_conflicts",
    "fmd_batch_debug_host_ms", "fmd_decoder_batch",
    "fmd_batch_enable_retune", "fmd_batch_retune_channels", "fmd_batch_debug_restart_skip",
    "fmd_batch_reset_channels", "fmd_batch_debug_reset_keep_ring_phase",
    "fmd_batch_set_capture_map", "fmd_batch_switch_captures", "fmd_batch_retune_channels_to",
    "fmd_batch_get_capture_map", "fmd_batch_debug_capture_walk",
    "fmd_scan_create", "fmd_scan_destroy", "fmd_scan_reset", "fmd_scan_slots", "fmd_scan_accumulate_device",
    "fmd_scan_accumulate_device_u8", "fmd_scan_accumulate_host", "fmd_scan_finish_device", "fmd_scan_finish_host",
    "fmd_batch_process_device_fmt", "fmd_batch_process_host_fmt", "fmd_process_stream_fmt", "fmd_receiver_write_fmt",
    "fmd_scan_accumulate_device_fmt", "fmd_scan_accumulate_host_fmt",
    "fmd_batch_process_device_pcm", "fmd_batch_process_host_pcm", "fmd_process_stream_pcm",
    "fmd_batch_read_pcm_clipped",
    "fmd_batch_process_device_mpx", "fmd_batch_process_host_mpx", "fmd_process_stream_mpx",
    "fmd_batch_max_mpx_samples", "fmd_batch_mpx_rate", "fmd_batch_debug_mpx_ms",
    "fmd_batch_state_size", "fmd_batch_save_state", "fmd_batch_load_state", "fmd_batch_export_channels",
    "fmd_batch_import_channels", "fmd_save_state", "fmd_load_state", "fmd_batch_debug_state_skip",
    "fmd_batch_set_feed", "fmd_batch_get_feed", "fmd_batch_feed_rate", "fmd_batch_max_feed_samples",
    "fmd_batch_get_feed_taps", "fmd_batch_process_device_feed", "fmd_batch_process_host_feed",
    "fmd_process_stream_feed", "fmd_batch_select_feed", "fmd_batch_get_feed_selection",
    "fmd_batch_debug_feed_skip_roll", "fmd_batch_baseband_limits", "fmd_batch_debug_ciq_in_skip_tile",
    "fmd_debug_ciq16_to_f32",
    "fmd_batch_process_device_call", "fmd_batch_process_host_call", "fmd_process_stream_call",
    "fmd_batch_select_ciq", "fmd_batch_get_ciq_selection",
    "fmd_batch_select_audio", "fmd_batch_select_mpx", "fmd_batch_get_audio_selection", "fmd_batch_get_mpx_selection",
    "fmd_batch_set_rds_blocks", "fmd_batch_get_rds_blocks", "fmd_batch_collect_rds_blocks",
    "fmd_batch_read_rds_quality",
    "fmd_batch_set_loudness", "fmd_batch_get_loudness", "fmd_batch_loudness_block_frames",
    "fmd_batch_get_loudness_coeffs", "fmd_batch_collect_loudness", "fmd_loudness_window", "fmd_loudness_integrated",
    "fmd_batch_debug_loud_skip_carry",
    "fmd_split_create", "fmd_split_destroy", "fmd_split_reset", "fmd_split_set_shifts", "fmd_split_rows",
    "fmd_split_out_rate", "fmd_split_max_out_samples", "fmd_split_get_taps", "fmd_split_tile_samples",
    "fmd_split_debug_table_versions", "fmd_split_process_device", "fmd_split_process_host",
    "fmd_split_create_real",
    "fmd_chan_create", "fmd_chan_destroy", "fmd_chan_reset", "fmd_chan_set_shifts", "fmd_chan_rows",
    "fmd_chan_out_rate", "fmd_chan_max_out_samples", "fmd_chan_get_taps", "fmd_chan_tile_samples",
    "fmd_chan_process_device", "fmd_chan_process_host",
    "fmd_chan_create_real", "fmd_chan_process_device_fmt", "fmd_chan_process_host_fmt",
]


def build():
    """Compile the HIP library for gfx950 (hipcc cross-compiles without a GPU)."""
    subprocess.check_call(["make", "-s", "-C", os.path.join(_HERE, "csrc")])


def lib():
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError("libfmd_hip.so is not built (run __graft_entry__.build()); "
                               "this package has no CPU fallback")
        # torch bundles its own libamdhip64 (same soname as /opt/rocm's).  Importing torch first
        # makes the loader bind this library to that already-loaded runtime, so device pointers,
        # streams and RCCL from torch and the kernels here share ONE HIP runtime per process.
        import torch  # noqa: F401
        L = C.CDLL(LIB_PATH)
        vp, u, i = C.c_void_p, C.c_uint, C.c_int
        L.fmd_last_error.restype = C.c_char_p
        L.fmd_version.restype = C.c_char_p
        L.fmd_stage_name.restype = C.c_char_p
        L.fmd_stage_name.argtypes = [u]
        L.fmd_create.argtypes = [C.POINTER(FmdParams), C.POINTER(FmdCallbacks), vp, C.POINTER(vp)]
        L.fmd_destroy.argtypes = [vp]
        L.fmd_reset.argtypes = [vp]
        L.fmd_process_stream.argtypes = [vp, vp, u, vp]
        L.fmd_process_stream_u8.argtypes = [vp, vp, u, vp]
        L.fmd_get_status.argtypes = [vp, C.POINTER(FmdStatus)]
        L.fmd_batch_create.argtypes = [C.POINTER(FmdParams), u, vp, i, C.POINTER(FmdCallbacks), vp,
                                       C.POINTER(vp)]
        L.fmd_batch_destroy.argtypes = [vp]
        L.fmd_batch_reset.argtypes = [vp]
        L.fmd_batch_enable_retune.argtypes = [vp]
        L.fmd_batch_retune_channels.argtypes = [vp, vp, vp, u]
        L.fmd_batch_debug_restart_skip.argtypes = [vp, i]
        L.fmd_batch_reset_channels.argtypes = [vp, vp, u]
        L.fmd_batch_debug_reset_keep_ring_phase.argtypes = [vp, i]
        L.fmd_batch_channels.restype = u
        L.fmd_batch_channels.argtypes = [vp]
        L.fmd_batch_min_samples.restype = u
        L.fmd_batch_min_samples.argtypes = [vp]
        L.fmd_batch_max_audio_floats.restype = u
        L.fmd_batch_max_audio_floats.argtypes = [vp, u]
        L.fmd_batch_process_device.argtypes = [vp, vp, C.c_size_t, u, vp, C.c_size_t,
                                               C.POINTER(u), vp]
        L.fmd_batch_process_host.argtypes = [vp, vp, C.c_size_t, u, vp, C.c_size_t, C.POINTER(u)]
        L.fmd_batch_process_device_u8.argtypes = L.fmd_batch_process_device.argtypes
        L.fmd_batch_process_host_u8.argtypes = L.fmd_batch_process_host.argtypes
        L.fmd_batch_collect_rds.argtypes = [vp, vp, u, i, vp]
        L.fmd_batch_collect_rds_lagged.argtypes = [vp, vp, u, i, i, vp]
        L.fmd_batch_export_rds_device.argtypes = [vp, vp, u, u, i, vp]
        L.fmd_batch_set_concurrency.argtypes = [vp, i]
        L.fmd_batch_set_channels_per_capture.argtypes = [vp, u]
        L.fmd_batch_set_capture_map.argtypes = [vp, vp, u]
        L.fmd_batch_switch_captures.argtypes = [vp, vp, vp, u]
        L.fmd_batch_retune_channels_to.argtypes = [vp, vp, vp, vp, u]
        L.fmd_batch_get_capture_map.argtypes = [vp, vp, u]
        L.fmd_batch_debug_capture_walk.argtypes = [vp, i]
        L.fmd_batch_streams_sharing_queue.argtypes = [vp]
        L.fmd_batch_wait.argtypes = [vp, vp]
        L.fmd_batch_wait_lagged.argtypes = [vp, i, vp]
        L.fmd_batch_get_status.argtypes = [vp, u, C.POINTER(FmdStatus)]
        L.fmd_batch_get_tap.argtypes = [vp, i, u, vp, u]
        L.fmd_batch_get_audio_level.argtypes = [vp, u, C.POINTER(FmdAudioLevel)]
        L.fmd_debug_math.argtypes = [i, u, vp, vp, vp, vp]
        L.fmd_batch_debug_serial_probe.argtypes = [vp, vp, u]
        L.fmd_batch_debug_stream_conflicts.argtypes = [vp, vp]
        L.fmd_design_lanczos.argtypes = [u, C.c_double, vp, u]
        L.fmd_design_lp_kaiser.argtypes = [C.c_float] * 5 + [vp, u]
        L.fmd_design_biquad.argtypes = [i, C.c_float, C.c_float, C.c_float, vp]
        L.fmd_design_tuner_lut.argtypes = [u, i, vp, u]
        L.fmd_receiver_open.argtypes = [C.POINTER(FmdParams), C.c_double, C.c_char_p, C.POINTER(vp)]
        L.fmd_receiver_close.argtypes = [vp]
        L.fmd_receiver_write_iq.argtypes = [vp, vp, u]
        L.fmd_receiver_write_u8.argtypes = [vp, vp, u]
        L.fmd_receiver_end.argtypes = [vp]
        L.fmd_receiver_queued_samples.restype = C.c_size_t
        L.fmd_receiver_queued_samples.argtypes = [vp]
        L.fmd_receiver_set_stream_change.argtypes = [vp]
        L.fmd_receiver_demux_read.argtypes = [vp, C.POINTER(FmdDemuxPacket)]
        L.fmd_receiver_signal_status.argtypes = [vp, C.POINTER(C.c_float), C.POINTER(C.c_float),
                                                 C.POINTER(i)]
        L.fmd_receiver_pvr_signal_status.argtypes = [vp, C.POINTER(FmdPvrSignalStatus)]
        L.fmd_receiver_decoder.restype = vp
        L.fmd_receiver_decoder.argtypes = [vp]
        L.fmd_batch_get_design.argtypes = [vp, i, vp, u]
        L.fmd_batch_set_profiling.argtypes = [vp, i]
        L.fmd_batch_set_debug_taps.argtypes = [vp, i]
        L.fmd_batch_get_stage_ms.argtypes = [vp, vp, u]
        L.fmd_group_decoder_create.restype = vp
        L.fmd_group_decoder_create.argtypes = [C.POINTER(FmdCallbacks), vp, u]
        L.fmd_group_decoder_destroy.argtypes = [vp]
        L.fmd_group_decoder_reset.argtypes = [vp]
        L.fmd_group_decoder_push.argtypes = [vp, vp]
        L.fmd_uecp_stuff_frame.argtypes = [vp, u, vp, u]
        L.fmd_batch_take_rds_lost.argtypes = [vp]
        L.fmd_batch_status_call_index.argtypes = [vp, u, C.POINTER(C.c_uint32)]
        L.fmd_batch_debug_set_spin_limit.argtypes = [vp, u]
        L.fmd_batch_debug_timeline.argtypes = [vp, vp, u]
        L.fmd_batch_debug_set.argtypes = [vp, C.c_char_p, i]
        L.fmd_batch_debug_host_ms.argtypes = [vp, vp]
        L.fmd_decoder_batch.restype = vp
        L.fmd_decoder_batch.argtypes = [vp]
        L.fmd_scan_create.argtypes = [C.POINTER(FmdScanParams), u, i, C.POINTER(vp)]
        L.fmd_scan_destroy.argtypes = [vp]
        L.fmd_scan_destroy.restype = None
        L.fmd_scan_reset.argtypes = [vp, vp]
        L.fmd_scan_slots.argtypes = [vp, C.POINTER(C.c_int32)]
        L.fmd_scan_accumulate_device.argtypes = [vp, vp, C.c_size_t, u, vp]
        L.fmd_scan_accumulate_device_u8.argtypes = [vp, vp, C.c_size_t, u, vp]
        L.fmd_scan_accumulate_host.argtypes = [vp, vp, C.c_size_t, u]
        L.fmd_scan_finish_device.argtypes = [vp, vp, vp, vp, vp, u, vp, vp]
        L.fmd_scan_finish_host.argtypes = [vp, vp, vp, vp, vp, u, vp]
        L.fmd_batch_process_device_fmt.argtypes = [vp, vp, i, C.c_size_t, u, vp, C.c_size_t, C.POINTER(u), vp]
        L.fmd_batch_process_host_fmt.argtypes = [vp, vp, i, C.c_size_t, u, vp, C.c_size_t, C.POINTER(u)]
        L.fmd_process_stream_fmt.argtypes = [vp, vp, i, u, vp]
        L.fmd_receiver_write_fmt.argtypes = [vp, vp, i, u]
        L.fmd_scan_accumulate_device_fmt.argtypes = [vp, vp, i, C.c_size_t, u, vp]
        L.fmd_scan_accumulate_host_fmt.argtypes = [vp, vp, i, C.c_size_t, u]
        L.fmd_batch_process_device_pcm.argtypes = [vp, vp, i, C.c_size_t, u, vp, i, C.c_size_t, C.POINTER(u), vp]
        L.fmd_batch_process_host_pcm.argtypes = [vp, vp, i, C.c_size_t, u, vp, i, C.c_size_t, C.POINTER(u)]
        L.fmd_process_stream_pcm.argtypes = [vp, vp, i, u, vp, i]
        L.fmd_batch_read_pcm_clipped.argtypes = [vp, u, u, vp]
        L.fmd_batch_process_device_mpx.argtypes = [vp, vp, i, C.c_size_t, u, vp, i, C.c_size_t, C.POINTER(u),
                                                   vp, i, C.c_size_t, C.POINTER(u), vp]
        L.fmd_batch_process_host_mpx.argtypes = [vp, vp, i, C.c_size_t, u, vp, i, C.c_size_t, C.POINTER(u),
                                                 vp, i, C.c_size_t, C.POINTER(u)]
        L.fmd_process_stream_mpx.argtypes = [vp, vp, i, u, vp, i, vp, i, C.POINTER(u)]
        L.fmd_batch_max_mpx_samples.restype = u
        L.fmd_batch_max_mpx_samples.argtypes = [vp, u]
        L.fmd_batch_mpx_rate.restype = C.c_double
        L.fmd_batch_mpx_rate.argtypes = [vp]
        L.fmd_batch_debug_mpx_ms.argtypes = [vp, vp, u]
        L.fmd_batch_state_size.restype = C.c_size_t
        L.fmd_batch_state_size.argtypes = [vp, u]
        L.fmd_batch_save_state.argtypes = [vp, vp, C.c_size_t, C.POINTER(C.c_size_t)]
        L.fmd_batch_load_state.argtypes = [vp, vp, C.c_size_t]
        L.fmd_batch_export_channels.argtypes = [vp, vp, u, vp, C.c_size_t, C.POINTER(C.c_size_t)]
        L.fmd_batch_import_channels.argtypes = [vp, vp, u, vp, C.c_size_t]
        L.fmd_save_state.argtypes = [vp, vp, C.c_size_t, C.POINTER(C.c_size_t)]
        L.fmd_load_state.argtypes = [vp, vp, C.c_size_t]
        L.fmd_batch_debug_state_skip.argtypes = [vp, i]
        L.fmd_batch_select_audio.argtypes = [vp, vp, u]
        L.fmd_batch_select_mpx.argtypes = [vp, vp, u]
        L.fmd_batch_set_feed.argtypes = [vp, i]
        L.fmd_batch_get_feed.argtypes = [vp]
        L.fmd_batch_feed_rate.restype = C.c_double
        L.fmd_batch_feed_rate.argtypes = [vp]
        L.fmd_batch_max_feed_samples.restype = u
        L.fmd_batch_max_feed_samples.argtypes = [vp, u]
        L.fmd_batch_get_feed_taps.argtypes = [vp, vp, u]
        L.fmd_batch_process_device_feed.argtypes = [vp, vp, i, C.c_size_t, u, vp, i, C.c_size_t, C.POINTER(u),
                                                    vp, i, C.c_size_t, C.POINTER(u),
                                                    vp, i, C.c_size_t, C.POINTER(u), vp]
        L.fmd_batch_process_host_feed.argtypes = [vp, vp, i, C.c_size_t, u, vp, i, C.c_size_t, C.POINTER(u),
                                                  vp, i, C.c_size_t, C.POINTER(u),
                                                  vp, i, C.c_size_t, C.POINTER(u)]
        L.fmd_process_stream_feed.argtypes = [vp, vp, i, u, vp, i, vp, i, C.POINTER(u)]
        L.fmd_batch_select_feed.argtypes = [vp, vp, u]
        L.fmd_batch_get_feed_selection.argtypes = [vp, vp, u]
        L.fmd_batch_debug_feed_skip_roll.argtypes = [vp, i]
        L.fmd_batch_baseband_limits.argtypes = [vp, vp, vp, vp]
        L.fmd_batch_debug_ciq_in_skip_tile.argtypes = [vp, i]
        L.fmd_debug_ciq16_to_f32.argtypes = [vp, u, vp]
        L.fmd_batch_process_device_call.argtypes = [vp, C.POINTER(FmdCall)]
        L.fmd_batch_process_host_call.argtypes = [vp, C.POINTER(FmdCall)]
        L.fmd_process_stream_call.argtypes = [vp, C.POINTER(FmdCall)]
        L.fmd_batch_select_ciq.argtypes = [vp, vp, u]
        L.fmd_batch_get_ciq_selection.argtypes = [vp, vp, u]
        L.fmd_batch_get_audio_selection.argtypes = [vp, vp, u]
        L.fmd_batch_get_mpx_selection.argtypes = [vp, vp, u]
        L.fmd_batch_set_rds_blocks.argtypes = [vp, i, u]
        L.fmd_batch_get_rds_blocks.argtypes = [vp]
        L.fmd_batch_collect_rds_blocks.argtypes = [vp, vp, u, i, vp, C.POINTER(u)]
        L.fmd_batch_read_rds_quality.argtypes = [vp, u, u, vp]
        L.fmd_batch_set_loudness.argtypes = [vp, i, u, u]
        L.fmd_batch_get_loudness.argtypes = [vp]
        L.fmd_batch_loudness_block_frames.restype = u
        L.fmd_batch_loudness_block_frames.argtypes = [vp]
        L.fmd_batch_get_loudness_coeffs.argtypes = [vp, vp]
        L.fmd_batch_collect_loudness.argtypes = [vp, vp, u, u, u, i, vp, C.POINTER(C.c_uint64), C.POINTER(u)]
        L.fmd_loudness_window.restype = C.c_double
        L.fmd_loudness_window.argtypes = [vp, u, u]
        L.fmd_loudness_integrated.restype = C.c_double
        L.fmd_loudness_integrated.argtypes = [vp, u, u]
        L.fmd_batch_debug_loud_skip_carry.argtypes = [vp, i]
        L.fmd_split_create.argtypes = [C.POINTER(FmdSplitParams), u, u, vp, i, C.POINTER(vp)]
        L.fmd_split_create_real.argtypes = [C.POINTER(FmdSplitParams), u, u, vp, i, C.POINTER(vp)]
        L.fmd_split_destroy.argtypes = [vp]
        L.fmd_split_destroy.restype = None
        L.fmd_split_reset.argtypes = [vp, vp]
        L.fmd_split_set_shifts.argtypes = [vp, vp, u]
        L.fmd_split_rows.argtypes = [vp]
        L.fmd_split_out_rate.restype = C.c_double
        L.fmd_split_out_rate.argtypes = [vp]
        L.fmd_split_max_out_samples.restype = u
        L.fmd_split_max_out_samples.argtypes = [vp, u]
        L.fmd_split_get_taps.argtypes = [vp, vp, u]
        L.fmd_split_tile_samples.restype = u
        L.fmd_split_tile_samples.argtypes = [vp]
        L.fmd_split_debug_table_versions.argtypes = [vp]
        L.fmd_split_process_device.argtypes = [vp, vp, i, C.c_size_t, u, vp, C.c_size_t, C.POINTER(u), vp]
        L.fmd_split_process_host.argtypes = [vp, vp, i, C.c_size_t, u, vp, C.c_size_t, C.POINTER(u)]
        L.fmd_chan_create.argtypes = [C.POINTER(FmdChanParams), u, u, vp, i, C.POINTER(vp)]
        L.fmd_chan_destroy.argtypes = [vp]
        L.fmd_chan_destroy.restype = None
        L.fmd_chan_reset.argtypes = [vp, vp]
        L.fmd_chan_set_shifts.argtypes = [vp, vp, u]
        L.fmd_chan_rows.argtypes = [vp]
        L.fmd_chan_out_rate.restype = C.c_double
        L.fmd_chan_out_rate.argtypes = [vp]
        L.fmd_chan_max_out_samples.restype = u
        L.fmd_chan_max_out_samples.argtypes = [vp, u]
        L.fmd_chan_get_taps.argtypes = [vp, vp, u]
        L.fmd_chan_tile_samples.restype = u
        L.fmd_chan_tile_samples.argtypes = [vp]
        L.fmd_chan_process_device.argtypes = [vp, vp, i, C.c_size_t, u, vp, C.c_size_t, C.POINTER(u), vp]
        L.fmd_chan_process_host.argtypes = [vp, vp, i, C.c_size_t, u, vp, C.c_size_t, C.POINTER(u)]
        L.fmd_chan_create_real.argtypes = [C.POINTER(FmdChanParams), u, u, vp, i, C.POINTER(vp)]
        L.fmd_chan_process_device_fmt.argtypes = [vp, vp, i, C.c_size_t, u, vp, i, C.c_size_t, C.POINTER(u), vp]
        L.fmd_chan_process_host_fmt.argtypes = [vp, vp, i, C.c_size_t, u, vp, i, C.c_size_t, C.POINTER(u)]
        _LIB = L
    return _LIB


class FmdError(RuntimeError):
    pass


def _check(rc):
    if rc < 0:
        raise FmdError("fmd error %d: %s" % (rc, lib().fmd_last_error().decode()))
    return rc


FMD_ERR_ARG_TEXT = "fmd error -1: %s"  # an argument the Python layer refuses itself, worded like _check's


def iq_format_of(arr):
    """(contiguous array, FMD_IQ_* format, array elements per IQ sample) by the array's dtype: complex64 (1 element
    per sample) or float32 / uint8 / int8 / int16 holding I, Q, I, Q, ... (2).  Any other dtype raises: nothing is
    converted silently."""
    a = np.ascontiguousarray(arr)
    if a.dtype == np.complex64:
        return a, FMD_IQ_F32, 1
    fmt = {np.dtype(np.float32): FMD_IQ_F32, np.dtype(np.uint8): FMD_IQ_U8, np.dtype(np.int8): FMD_IQ_S8,
           np.dtype(np.int16): FMD_IQ_S16}.get(a.dtype)
    if fmt is None:
        raise FmdError(FMD_ERR_ARG_TEXT % ("no IQ format for dtype %s (complex64, float32, uint8, int8, int16)"
                                           % a.dtype))
    return a, fmt, 2


def pcm_format_of(pcm):
    """FMD_PCM_* of a `pcm=` argument: None or np.float32 (the default output), np.int16, or the constant itself.
    Anything else raises: no other output format exists."""
    if pcm is None:
        return FMD_PCM_F32
    if isinstance(pcm, (int, np.integer)) and not isinstance(pcm, bool):
        if int(pcm) in PCM_BYTES:
            return int(pcm)
    else:
        try:
            fmt = {np.dtype(np.float32): FMD_PCM_F32, np.dtype(np.int16): FMD_PCM_S16}.get(np.dtype(pcm))
        except TypeError:
            fmt = None
        if fmt is not None:
            return fmt
    raise FmdError(FMD_ERR_ARG_TEXT % ("no audio format for %r (float32, int16, FMD_PCM_F32, FMD_PCM_S16)" % (pcm,)))


def feed_format_of(feed):
    """FMD_FEED_* of a `feed=` argument: np.float32, np.int16, or the constant itself.  Anything else raises: no
    silent conversion."""
    if isinstance(feed, (int, np.integer)) and not isinstance(feed, bool):
        if int(feed) in FEED_BYTES:
            return int(feed)
    elif feed is not None:
        try:
            fmt = {np.dtype(np.float32): FMD_FEED_F32, np.dtype(np.int16): FMD_FEED_S16}.get(np.dtype(feed))
        except TypeError:
            fmt = None
        if fmt is not None:
            return fmt
    raise FmdError(FMD_ERR_ARG_TEXT % ("no feed format for %r (float32, int16, FMD_FEED_F32, FMD_FEED_S16)"
                                       % (feed,)))


def ciq_format_of(ciq):
    """FMD_CIQ_* of a `ciq=` argument: np.complex64, np.int16, or the constant itself.  Anything else raises: no
    format is guessed."""
    if isinstance(ciq, (int, np.integer)) and not isinstance(ciq, bool):
        if int(ciq) in CIQ_BYTES:
            return int(ciq)
    elif ciq is not None:
        try:
            fmt = {np.dtype(np.complex64): FMD_CIQ_F32, np.dtype(np.int16): FMD_CIQ_S16}.get(np.dtype(ciq))
        except TypeError:
            fmt = None
        if fmt is not None:
            return fmt
    raise FmdError(FMD_ERR_ARG_TEXT % ("no channel IQ format for %r (complex64, int16, FMD_CIQ_F32, FMD_CIQ_S16)"
                                       % (ciq,)))


def _ciq_rows(fmt, rows, stride):
    """host rows for the channel IQ: complex64 [rows, stride], or int16 [rows, stride, 2] (re, im)"""
    if fmt == FMD_CIQ_S16:
        return np.zeros((rows, stride, 2), dtype=np.int16)
    return np.zeros((rows, stride), dtype=np.complex64)


def mpx_format_of(mpx):
    """FMD_MPX_* of an `mpx=` argument: np.float32, np.int16, or the constant itself.  Anything else raises: no
    other multiplex format exists (None is no format: the caller did not ask for the multiplex)."""
    if isinstance(mpx, (int, np.integer)) and not isinstance(mpx, bool):
        if int(mpx) in MPX_BYTES:
            return int(mpx)
    elif mpx is not None:
        try:
            fmt = {np.dtype(np.float32): FMD_MPX_F32, np.dtype(np.int16): FMD_MPX_S16}.get(np.dtype(mpx))
        except TypeError:
            fmt = None
        if fmt is not None:
            return fmt
    raise FmdError(FMD_ERR_ARG_TEXT % ("no multiplex format for %r (float32, int16, FMD_MPX_F32, FMD_MPX_S16)"
                                       % (mpx,)))


FIR_SEQUENTIAL = 0
FIR_SHUFFLE_PARITY_WAIVED = 0x101  # include/fmd.h: the shuffle-reduced IF FIR, outside the parity contract
FIR_FMA_PARITY_WAIVED = 0x102  # FMD_FIR_FMA_PARITY_WAIVED: fused multiply-add, the reference's tap order


def make_params(sample_rate_if, tuning_offset, sample_rate_pcm=48000.0, bandwidth_pcm=15000.0,
                downsample=1, us_version=False, table_size=0, if_filter_order=0, fir_reduction=0):
    return FmdParams(sample_rate_if, tuning_offset, sample_rate_pcm, bandwidth_pcm, downsample,
                     int(us_version), table_size, if_filter_order, fir_reduction)


class _CallbackSink:
    """Python stand-in for the three cRadioReceiver callbacks; records what arrives."""

    def __init__(self):
        self.frames = {}
        self.names = {}
        self.setting_active = False

        def on_frame(_user, ch, data, n):
            self.frames.setdefault(ch, []).append(bytes(data[:n]))
            return 1

        def on_name(_user, ch, name):
            self.names[ch] = name[:8].decode("latin1")
            return 1

        def on_active(_user, ch):
            return 1 if self.setting_active else 0

        self.struct = FmdCallbacks(UECP_CB(on_frame), NAME_CB(on_name), ACTIVE_CB(on_active))


class Batch:
    """C channels of the FM decoder on one GPU (fmd_batch_*)."""

    def __init__(self, params, n_channels, tuning_shifts=None, device=0, record_callbacks=True):
        self.sink = _CallbackSink() if record_callbacks else None
        h = C.c_void_p()
        shifts = None
        if tuning_shifts is not None:
            shifts = np.ascontiguousarray(tuning_shifts, dtype=np.int32)
            assert shifts.size == n_channels
        _check(lib().fmd_batch_create(
            C.byref(params), n_channels, shifts.ctypes.data if shifts is not None else None, device,
            C.byref(self.sink.struct) if self.sink else None, None, C.byref(h)))
        self._h = h
        self.n_channels = n_channels

    def close(self):
        if getattr(self, "_h", None):
            lib().fmd_batch_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()

    def reset(self):
        _check(lib().fmd_batch_reset(self._h))

    def enable_retune(self):
        """Opt in to retune() (fmd_batch_enable_retune): only before the first call."""
        _check(lib().fmd_batch_enable_retune(self._h))

    def retune(self, channels, shifts, captures=None):
        """Move channels to new tuner shifts from the next call on (fmd_batch_retune_channels): each then decodes
        like a decoder created with that shift that received zeros until now.  With `captures`, each also reads
        that capture from the next call on (fmd_batch_retune_channels_to)."""
        ch = np.ascontiguousarray(channels, dtype=np.uint32).reshape(-1)
        sh = np.ascontiguousarray(shifts, dtype=np.int32).reshape(-1)
        assert ch.size == sh.size
        if captures is None:
            _check(lib().fmd_batch_retune_channels(self._h, ch.ctypes.data, sh.ctypes.data, ch.size))
            return
        cp = np.ascontiguousarray(captures, dtype=np.uint32).reshape(-1)
        assert cp.size == ch.size
        _check(lib().fmd_batch_retune_channels_to(self._h, ch.ctypes.data, sh.ctypes.data, cp.ctypes.data, ch.size))

    def set_capture_map(self, capture_of, n_captures):
        """Channel c reads input row capture_of[c] of n_captures (fmd_batch_set_capture_map); None: one row per
        channel.  The process calls then take [n_captures, N] rows."""
        if capture_of is None:
            _check(lib().fmd_batch_set_capture_map(self._h, None, 0))
        else:
            m = np.ascontiguousarray(capture_of, dtype=np.uint32).reshape(-1)
            assert m.size == self.n_channels
            _check(lib().fmd_batch_set_capture_map(self._h, m.ctypes.data, int(n_captures)))
        self.channels_per_capture = 1

    def switch_captures(self, channels, captures):
        """From the next call on, channels[i] reads captures[i] with all its state carried over
        (fmd_batch_switch_captures)."""
        ch = np.ascontiguousarray(channels, dtype=np.uint32).reshape(-1)
        cp = np.ascontiguousarray(captures, dtype=np.uint32).reshape(-1)
        assert ch.size == cp.size
        _check(lib().fmd_batch_switch_captures(self._h, ch.ctypes.data, cp.ctypes.data, ch.size))

    def capture_map(self):
        """(capture of every channel as the next call reads it, number of input rows) (fmd_batch_get_capture_map)."""
        out = np.zeros(self.n_channels, dtype=np.uint32)
        n = _check(lib().fmd_batch_get_capture_map(self._h, out.ctypes.data, out.size))
        return out, n

    def debug_capture_walk(self, on):
        """Development switch: the map form's IF stage walks the channels sorted by capture (1, default) or in channel
        order (0) (fmd_batch_debug_capture_walk)."""
        _check(lib().fmd_batch_debug_capture_walk(self._h, int(on)))

    def _input_rows(self):
        return _check(lib().fmd_batch_get_capture_map(self._h, None, 0))

    def reset_channels(self, channels):
        """Reset single channels from the next call on (fmd_batch_reset_channels): each then decodes like its own
        decoder after cFmDecoder::Reset() in front of that call; the other channels do not notice."""
        ch = np.ascontiguousarray(channels, dtype=np.uint32).reshape(-1)
        _check(lib().fmd_batch_reset_channels(self._h, ch.ctypes.data, ch.size))

    def debug_reset_keep_ring_phase(self, on):
        """Test aid: resets that follow leave the ring origins at the batch's phase (not exact)."""
        _check(lib().fmd_batch_debug_reset_keep_ring_phase(self._h, int(on)))

    def debug_restart_skip(self, region):
        """Test aid: leave one carried region out of the restarts (fmd_batch_debug_restart_skip); -1 = none."""
        _check(lib().fmd_batch_debug_restart_skip(self._h, region))

    def save_state(self):
        """The whole batch as an opaque blob (fmd_batch_save_state): waits for every call submitted so far and
        changes nothing.  load_state of it into a batch of the same geometry and channel count continues bit for
        bit.  RDS groups still queued are not carried: collect them first."""
        buf = np.empty(lib().fmd_batch_state_size(self._h, self.n_channels), dtype=np.uint8)
        n = C.c_size_t()
        _check(lib().fmd_batch_save_state(self._h, buf.ctypes.data, buf.size, C.byref(n)))
        return buf[:n.value].tobytes()

    def load_state(self, blob):
        """Replace the whole state and the clock by a save_state blob (fmd_batch_load_state)."""
        buf = np.frombuffer(blob, dtype=np.uint8)
        _check(lib().fmd_batch_load_state(self._h, buf.ctypes.data if buf.size else None, buf.size))

    def export_channels(self, channels):
        """The listed channels' decoders as a blob, in list order (fmd_batch_export_channels)."""
        ch = np.ascontiguousarray(channels, dtype=np.uint32).reshape(-1)
        buf = np.empty(lib().fmd_batch_state_size(self._h, max(1, ch.size)), dtype=np.uint8)
        n = C.c_size_t()
        _check(lib().fmd_batch_export_channels(self._h, ch.ctypes.data, ch.size, buf.ctypes.data, buf.size,
                                               C.byref(n)))
        return buf[:n.value].tobytes()

    def import_channels(self, channels, blob):
        """From the next call on, slot channels[i] is the decoder of the blob's record i
        (fmd_batch_import_channels); the batch's clock must equal the blob's."""
        ch = np.ascontiguousarray(channels, dtype=np.uint32).reshape(-1)
        buf = np.frombuffer(blob, dtype=np.uint8)
        _check(lib().fmd_batch_import_channels(self._h, ch.ctypes.data, ch.size,
                                               buf.ctypes.data if buf.size else None, buf.size))

    def debug_state_skip(self, region):
        """Test aid: loads and imports that follow leave one region out (fmd_batch_debug_state_skip); -1 = none."""
        _check(lib().fmd_batch_debug_state_skip(self._h, int(region)))

    def _selection_list(self, channels, what):
        """The list of a select_* call as uint32, refused here like the library refuses it (before any device call)."""
        ch = np.asarray(channels, dtype=np.int64).reshape(-1)
        if ch.size > self.n_channels:
            raise FmdError(FMD_ERR_ARG_TEXT % ("%s: more rows than the batch has channels" % what))
        if ch.size and (ch.min() < 0 or ch.max() >= self.n_channels):
            raise FmdError(FMD_ERR_ARG_TEXT % ("%s: a channel is out of range" % what))
        if np.unique(ch).size != ch.size:
            raise FmdError(FMD_ERR_ARG_TEXT % ("%s: a channel is listed twice" % what))
        return np.ascontiguousarray(ch, dtype=np.uint32)

    def select_audio(self, channels):
        """From the next call on, audio row i is channel channels[i] and the call writes len(channels) rows
        (fmd_batch_select_audio); None: one row per channel again; an empty list: no audio rows."""
        if channels is None:
            _check(lib().fmd_batch_select_audio(self._h, None, 0))
            return
        ch = self._selection_list(channels, "select_audio")
        keep = ch if ch.size else np.zeros(1, dtype=np.uint32)  # (an empty list is still a list: a non-null pointer)
        _check(lib().fmd_batch_select_audio(self._h, keep.ctypes.data, ch.size))

    def select_mpx(self, channels):
        """The same for the multiplex rows (fmd_batch_select_mpx)."""
        if channels is None:
            _check(lib().fmd_batch_select_mpx(self._h, None, 0))
            return
        ch = self._selection_list(channels, "select_mpx")
        keep = ch if ch.size else np.zeros(1, dtype=np.uint32)
        _check(lib().fmd_batch_select_mpx(self._h, keep.ctypes.data, ch.size))

    def select_feed(self, channels):
        """The same for the feed rows (fmd_batch_select_feed); an empty list: no rows are written, the feed's history
        and frame count go on."""
        if channels is None:
            _check(lib().fmd_batch_select_feed(self._h, None, 0))
            return
        ch = self._selection_list(channels, "select_feed")
        keep = ch if ch.size else np.zeros(1, dtype=np.uint32)
        _check(lib().fmd_batch_select_feed(self._h, keep.ctypes.data, ch.size))

    def feed_selection(self):
        """uint32[n]: the channels of the feed rows the next call writes (fmd_batch_get_feed_selection)."""
        out = np.zeros(self.n_channels, dtype=np.uint32)
        n = _check(lib().fmd_batch_get_feed_selection(self._h, out.ctypes.data, out.size))
        return out[:n].copy()

    def set_feed(self, divisor):
        """Turn the mono feed at sample_rate_pcm / divisor on (2 or 3) or off (0): fmd_batch_set_feed.  A setup call:
        it waits for the calls in flight, zeroes the feed's history and starts its frame count at 0."""
        _check(lib().fmd_batch_set_feed(self._h, int(divisor)))

    def feed(self):
        """The feed's divisor, 0 while it is off (fmd_batch_get_feed)."""
        return _check(lib().fmd_batch_get_feed(self._h))

    def feed_rate(self):
        """Feed samples per second: sample_rate_pcm / divisor (fmd_batch_feed_rate)."""
        return lib().fmd_batch_feed_rate(self._h)

    def max_feed_samples(self, samples):
        """Feed samples per channel a call of `samples` delivers at most (fmd_batch_max_feed_samples)."""
        return lib().fmd_batch_max_feed_samples(self._h, samples)

    def feed_taps(self):
        """float32[T]: the feed's low-pass taps in use (fmd_batch_get_feed_taps)."""
        out = np.zeros(80, dtype=np.float32)
        n = _check(lib().fmd_batch_get_feed_taps(self._h, out.ctypes.data, out.size))
        return out[:n].copy()

    def debug_feed_skip_roll(self, on):
        """Test aid: leave out the roll of the feed's history (fmd_batch_debug_feed_skip_roll)."""
        _check(lib().fmd_batch_debug_feed_skip_roll(self._h, int(on)))

    def audio_selection(self):
        """uint32[n]: the channels of the audio rows the next call writes (fmd_batch_get_audio_selection)."""
        out = np.zeros(self.n_channels, dtype=np.uint32)
        n = _check(lib().fmd_batch_get_audio_selection(self._h, out.ctypes.data, out.size))
        return out[:n].copy()

    def mpx_selection(self):
        """uint32[n]: the channels of the multiplex rows the next call writes (fmd_batch_get_mpx_selection)."""
        out = np.zeros(self.n_channels, dtype=np.uint32)
        n = _check(lib().fmd_batch_get_mpx_selection(self._h, out.ctypes.data, out.size))
        return out[:n].copy()

    def select_ciq(self, channels):
        """The same for the channel IQ rows (fmd_batch_select_ciq); an empty list: the call without them."""
        if channels is None:
            _check(lib().fmd_batch_select_ciq(self._h, None, 0))
            return
        ch = self._selection_list(channels, "select_ciq")
        keep = ch if ch.size else np.zeros(1, dtype=np.uint32)
        _check(lib().fmd_batch_select_ciq(self._h, keep.ctypes.data, ch.size))

    def ciq_selection(self):
        """uint32[n]: the channels of the channel IQ rows the next call writes (fmd_batch_get_ciq_selection)."""
        out = np.zeros(self.n_channels, dtype=np.uint32)
        n = _check(lib().fmd_batch_get_ciq_selection(self._h, out.ctypes.data, out.size))
        return out[:n].copy()

    def process_call(self, call=None, ciq_in=None, **rows):
        """One device call from a call record (make_call; fmd_batch_process_device_call): the only way to the channel
        IQ rows (call.ciq: FMD_CIQ_*, stride and count in complex samples) and to channel IQ rows as the input.
        ciq_in: a device tensor of such rows (complex64 [C, M] or int16 [C, M, 2]: make_call's ciq_in) -- into the
        record given, or into a new one of the keyword arguments (audio=, mpx=, feed=, ciq=, stream=)."""
        if ciq_in is not None:
            ptr, fmt, stride, m = ciq_in_of(ciq_in)
            if call is None:
                call = make_call(ciq_in=ciq_in, **rows)
            else:
                call.iq, call.iq_format, call.iq_channel_stride, call.samples = ptr, fmt, stride, m
        _check(lib().fmd_batch_process_device_call(self._h, C.byref(call)))

    def baseband_limits(self):
        """(min, max, multiple) of the baseband length M of a call with channel IQ rows as input
        (fmd_batch_baseband_limits)."""
        lo, hi, mult = C.c_uint(), C.c_uint(), C.c_uint()
        _check(lib().fmd_batch_baseband_limits(self._h, C.byref(lo), C.byref(hi), C.byref(mult)))
        return lo.value, hi.value, mult.value

    def debug_ciq_in_skip_tile(self, on=True):
        """Test aid: the input copy of FMD_IN_CIQ_* leaves out a tile (fmd_batch_debug_ciq_in_skip_tile)."""
        _check(lib().fmd_batch_debug_ciq_in_skip_tile(self._h, int(on)))

    def process_host_ciq_in(self, ciq_in, pcm=None, mpx=None, feed=None, ciq=None):
        """One host call with channel IQ rows as the input (fmd_batch_process_host_call, FMD_IN_CIQ_*): ciq_in is
        complex64 [C, M] or int16 [C, M, 2], any row stride.  Returns the audio, or a tuple of it and the multiplex,
        feed and channel IQ rows asked for, as process_host_fmt does."""
        ptr, fmt, stride, m = ciq_in_of(ciq_in)
        pcm_fmt = pcm_format_of(pcm)
        n = 65536  # (the largest block: its bounds hold for every baseband length a call may have)
        a_stride, m_stride = self.max_audio_floats(n), max(m, 1)
        audio = np.zeros((self._rows(), a_stride), dtype=np.int16 if pcm_fmt == FMD_PCM_S16 else np.float32)
        nf, nm, nfeed, nq = C.c_uint(), C.c_uint(), C.c_uint(), C.c_uint()
        call = make_call(ptr, fmt, stride, m, audio=make_rows(audio.ctypes.data, pcm_fmt, a_stride, nf))
        out = []
        if mpx is not None:
            mpx_fmt = mpx_format_of(mpx)
            rows = np.zeros((self._rows(mpx=True), m_stride), dtype=np.int16 if mpx_fmt == FMD_MPX_S16 else np.float32)
            call.mpx = make_rows(rows.ctypes.data, mpx_fmt, m_stride, nm)
            out.append((rows, nm, None))
        if feed is not None:
            feed_fmt = feed_format_of(feed)
            f_stride = max(self.max_feed_samples(n), 1)
            frows = np.zeros((max(self._rows(feed=True), 1), f_stride),
                             dtype=np.int16 if feed_fmt == FMD_FEED_S16 else np.float32)
            call.feed = make_rows(frows.ctypes.data, feed_fmt, f_stride, nfeed)
            out.append((frows, nfeed, self._rows(feed=True)))
        if ciq is not None:
            ciq_fmt = ciq_format_of(ciq)
            qrows = _ciq_rows(ciq_fmt, max(self._rows(ciq=True), 1), m_stride)
            call.ciq = make_rows(qrows.ctypes.data, ciq_fmt, m_stride, nq)
            out.append((qrows, nq, self._rows(ciq=True)))
        _check(lib().fmd_batch_process_host_call(self._h, C.byref(call)))
        res = (audio[:, :nf.value],) + tuple(r[:r.shape[0] if k is None else k, :c.value] for r, c, k in out)
        return res[0] if len(res) == 1 else res

    def _rows(self, mpx=False, feed=False, ciq=False):
        if ciq:
            return _check(lib().fmd_batch_get_ciq_selection(self._h, None, 0))
        fn = (lib().fmd_batch_get_feed_selection if feed else
              lib().fmd_batch_get_mpx_selection if mpx else lib().fmd_batch_get_audio_selection)
        return _check(fn(self._h, None, 0))

    def min_samples(self):
        """Smallest call size this batch's geometry accepts (fmd_batch_min_samples)."""
        return lib().fmd_batch_min_samples(self._h)

    def max_audio_floats(self, samples):
        return lib().fmd_batch_max_audio_floats(self._h, samples)

    def max_mpx_samples(self, samples):
        """Multiplex samples per channel a call of `samples` delivers at most (fmd_batch_max_mpx_samples)."""
        return lib().fmd_batch_max_mpx_samples(self._h, samples)

    def mpx_rate(self):
        """Multiplex samples per second: sample_rate_if / downsample (fmd_batch_mpx_rate)."""
        return lib().fmd_batch_mpx_rate(self._h)

    def process_host(self, iq, shared=False):
        """iq: [C, N] complex64 ([captures, N] with several channels per capture or a capture map; [N] when
        shared).  Returns [C, n_floats] float32 audio."""
        iq = np.ascontiguousarray(iq)
        if iq.dtype != np.complex64:
            iq = iq.astype(np.float32).view(np.complex64)
        if shared:
            n = iq.size
            stride = 0
        else:
            iq = iq.reshape(self._input_rows(), -1)
            n = iq.shape[1]
            stride = n
        a_stride = self.max_audio_floats(n)
        audio = np.zeros((self._rows(), a_stride), dtype=np.float32)
        nf = C.c_uint()
        _check(lib().fmd_batch_process_host(self._h, iq.ctypes.data, stride, n, audio.ctypes.data,
                                            a_stride, C.byref(nf)))
        return audio[:, :nf.value]

    def process_host_u8(self, iq_u8, shared=False):
        """iq_u8: [C, 2N] uint8 RTL-SDR byte pairs (or [2N] when shared).  Same result as
        process_host on the converted block (RTL_SDR_Source.cpp:207-211)."""
        iq_u8 = np.ascontiguousarray(iq_u8, dtype=np.uint8)
        if shared:
            n = iq_u8.size // 2
            stride = 0
        else:
            iq_u8 = iq_u8.reshape(self._input_rows(), -1)
            n = iq_u8.shape[1] // 2
            stride = n
        a_stride = self.max_audio_floats(n)
        audio = np.zeros((self._rows(), a_stride), dtype=np.float32)
        nf = C.c_uint()
        _check(lib().fmd_batch_process_host_u8(self._h, iq_u8.ctypes.data, stride, n,
                                               audio.ctypes.data, a_stride, C.byref(nf)))
        return audio[:, :nf.value]

    def process_host_fmt(self, iq, shared=False, pcm=None, mpx=None, feed=None, ciq=None):
        """iq: [C, N] complex64, or [C, 2N] float32 / uint8 / int8 / int16 holding I, Q, I, Q, ... (rows as for
        process_host; one row when shared); the input format is the array's dtype (fmd_batch_process_host_fmt).
        Signed integers are v * 2^-7 / v * 2^-15: the same bits as process_host on the converted block.
        With a selection (select_audio / select_mpx) the arrays hold its rows, in its order.
        pcm=np.int16: the audio as int16 (FMD_PCM_S16, fmd_batch_process_host_pcm).
        mpx=np.float32 / np.int16: returns (audio, multiplex), the multiplex as [C, M] rows of that format
        (FMD_MPX_*, fmd_batch_process_host_mpx: a deviation of f Hz reads f / 30 000, times 8192 as int16).
        feed=np.int16 / np.float32: also returns the mono feed as [C, n] rows of that format, last of the tuple
        (FMD_FEED_*, fmd_batch_process_host_feed; set_feed turns the feed on).
        ciq=np.complex64 / np.int16: also returns the channel IQ, last of the tuple, as complex64 [C, M] rows or int16
        [C, M, 2] (re, im) rows (FMD_CIQ_*, through a call record: fmd_batch_process_host_call)."""
        if ciq is not None:
            return self._process_host_call(iq, shared, pcm, mpx, feed, ciq)
        iq, fmt, per = iq_format_of(iq)
        pcm_fmt = pcm_format_of(pcm)
        mpx_fmt = None if mpx is None else mpx_format_of(mpx)
        if shared:
            n = iq.size // per
            stride = 0
        else:
            iq = iq.reshape(self._input_rows(), -1)
            n = iq.shape[1] // per
            stride = n
        a_stride = self.max_audio_floats(n)
        audio = np.zeros((self._rows(), a_stride), dtype=np.int16 if pcm_fmt == FMD_PCM_S16 else np.float32)
        nf = C.c_uint()
        if feed is not None:
            feed_fmt = feed_format_of(feed)
            m_stride = self.max_mpx_samples(n) if mpx_fmt is not None else 0
            rows = (np.zeros((self._rows(mpx=True), m_stride), dtype=np.int16 if mpx_fmt == FMD_MPX_S16 else np.float32)
                    if mpx_fmt is not None else None)
            f_stride = max(self.max_feed_samples(n), 1)
            frows = np.zeros((max(self._rows(feed=True), 1), f_stride),
                             dtype=np.int16 if feed_fmt == FMD_FEED_S16 else np.float32)
            nm, nfeed = C.c_uint(), C.c_uint()
            _check(lib().fmd_batch_process_host_feed(self._h, iq.ctypes.data, fmt, stride, n, audio.ctypes.data,
                                                     pcm_fmt, a_stride, C.byref(nf),
                                                     None if rows is None else rows.ctypes.data,
                                                     FMD_MPX_F32 if mpx_fmt is None else mpx_fmt, m_stride,
                                                     C.byref(nm), frows.ctypes.data, feed_fmt, f_stride,
                                                     C.byref(nfeed)))
            frows = frows[:self._rows(feed=True), :nfeed.value]
            if rows is None:
                return audio[:, :nf.value], frows
            return audio[:, :nf.value], rows[:, :nm.value], frows
        if mpx_fmt is not None:
            m_stride = self.max_mpx_samples(n)
            rows = np.zeros((self._rows(mpx=True), m_stride), dtype=np.int16 if mpx_fmt == FMD_MPX_S16 else np.float32)
            nm = C.c_uint()
            _check(lib().fmd_batch_process_host_mpx(self._h, iq.ctypes.data, fmt, stride, n, audio.ctypes.data,
                                                    pcm_fmt, a_stride, C.byref(nf), rows.ctypes.data, mpx_fmt,
                                                    m_stride, C.byref(nm)))
            return audio[:, :nf.value], rows[:, :nm.value]
        if pcm is None:
            _check(lib().fmd_batch_process_host_fmt(self._h, iq.ctypes.data, fmt, stride, n, audio.ctypes.data,
                                                    a_stride, C.byref(nf)))
        else:
            _check(lib().fmd_batch_process_host_pcm(self._h, iq.ctypes.data, fmt, stride, n, audio.ctypes.data,
                                                    pcm_fmt, a_stride, C.byref(nf)))
        return audio[:, :nf.value]

    def _process_host_call(self, iq, shared, pcm, mpx, feed, ciq):
        """process_host_fmt with the channel IQ: the same outputs through one call record."""
        iq, fmt, per = iq_format_of(iq)
        pcm_fmt, ciq_fmt = pcm_format_of(pcm), ciq_format_of(ciq)
        if shared:
            n, stride = iq.size // per, 0
        else:
            iq = iq.reshape(self._input_rows(), -1)
            n = iq.shape[1] // per
            stride = n
        a_stride, m_stride = self.max_audio_floats(n), self.max_mpx_samples(n)
        audio = np.zeros((self._rows(), a_stride), dtype=np.int16 if pcm_fmt == FMD_PCM_S16 else np.float32)
        nf, nm, nfeed, nq = C.c_uint(), C.c_uint(), C.c_uint(), C.c_uint()
        call = make_call(iq.ctypes.data, fmt, stride, n, audio=make_rows(audio.ctypes.data, pcm_fmt, a_stride, nf))
        out = []
        if mpx is not None:
            mpx_fmt = mpx_format_of(mpx)
            rows = np.zeros((self._rows(mpx=True), m_stride), dtype=np.int16 if mpx_fmt == FMD_MPX_S16 else np.float32)
            call.mpx = make_rows(rows.ctypes.data, mpx_fmt, m_stride, nm)
            out.append((rows, nm, None))
        if feed is not None:
            feed_fmt = feed_format_of(feed)
            f_stride = max(self.max_feed_samples(n), 1)
            frows = np.zeros((max(self._rows(feed=True), 1), f_stride),
                             dtype=np.int16 if feed_fmt == FMD_FEED_S16 else np.float32)
            call.feed = make_rows(frows.ctypes.data, feed_fmt, f_stride, nfeed)
            out.append((frows, nfeed, self._rows(feed=True)))
        qrows = _ciq_rows(ciq_fmt, max(self._rows(ciq=True), 1), m_stride)
        call.ciq = make_rows(qrows.ctypes.data, ciq_fmt, m_stride, nq)
        out.append((qrows, nq, self._rows(ciq=True)))
        _check(lib().fmd_batch_process_host_call(self._h, C.byref(call)))
        return (audio[:, :nf.value],) + tuple(r[:r.shape[0] if k is None else k, :c.value] for r, c, k in out)

    def process_device(self, d_iq_ptr, iq_stride, samples, d_audio_ptr, audio_stride, stream=None,
                       u8=False, fmt=None, pcm=None, d_mpx_ptr=None, mpx_stride=0, mpx=None, d_feed_ptr=None,
                       feed_stride=0, feed=None, d_ciq_ptr=None, ciq_stride=0, ciq=None):
        """iq_stride in IQ samples; u8=True: d_iq_ptr holds RTL-SDR byte pairs; fmt (FMD_IQ_*): the input format,
        through fmd_batch_process_device_fmt; pcm (np.int16 / FMD_PCM_*): the output format, audio_stride and the
        returned count in its elements, through fmd_batch_process_device_pcm.
        d_mpx_ptr / mpx_stride / mpx (np.float32, np.int16 / FMD_MPX_*): the call's multiplex rows, through
        fmd_batch_process_device_mpx; returns (audio samples, multiplex samples) per channel.
        d_feed_ptr / feed_stride / feed (np.int16, np.float32 / FMD_FEED_*): the call's feed rows, through
        fmd_batch_process_device_feed; the feed samples per channel are the last of the returned tuple.
        d_ciq_ptr / ciq_stride / ciq (np.complex64, np.int16 / FMD_CIQ_*): the call's channel IQ rows, stride and
        count in complex samples, through a call record (fmd_batch_process_device_call); their count is the last of
        the returned tuple, behind the multiplex's and the feed's where those were asked for."""
        nf = C.c_uint()
        if d_ciq_ptr is not None or ciq is not None:
            in_fmt = int(fmt) if fmt is not None else FMD_IQ_U8 if u8 else FMD_IQ_F32
            nm, nfeed, nq = C.c_uint(), C.c_uint(), C.c_uint()
            want_mpx = d_mpx_ptr is not None or mpx is not None
            want_feed = d_feed_ptr is not None or feed is not None
            call = make_call(d_iq_ptr, in_fmt, iq_stride, samples, stream=stream,
                             audio=make_rows(d_audio_ptr, pcm_format_of(pcm), audio_stride, nf),
                             mpx=make_rows(d_mpx_ptr, mpx_format_of(FMD_MPX_F32 if mpx is None else mpx), mpx_stride, nm),
                             feed=make_rows(d_feed_ptr, feed_format_of(FMD_FEED_S16 if feed is None else feed),
                                            feed_stride, nfeed),
                             ciq=make_rows(d_ciq_ptr, ciq_format_of(FMD_CIQ_F32 if ciq is None else ciq), ciq_stride,
                                           nq))
            self.process_call(call)
            return ((nf.value,) + ((nm.value,) if want_mpx else ()) + ((nfeed.value,) if want_feed else ())
                    + (nq.value,))
        if d_feed_ptr is not None or feed is not None:
            in_fmt = int(fmt) if fmt is not None else FMD_IQ_U8 if u8 else FMD_IQ_F32
            nm, nfeed = C.c_uint(), C.c_uint()
            _check(lib().fmd_batch_process_device_feed(self._h, d_iq_ptr, in_fmt, iq_stride, samples, d_audio_ptr,
                                                       pcm_format_of(pcm), audio_stride, C.byref(nf), d_mpx_ptr,
                                                       mpx_format_of(FMD_MPX_F32 if mpx is None else mpx), mpx_stride,
                                                       C.byref(nm), d_feed_ptr,
                                                       feed_format_of(FMD_FEED_S16 if feed is None else feed),
                                                       feed_stride, C.byref(nfeed), stream))
            if d_mpx_ptr is not None or mpx is not None:
                return nf.value, nm.value, nfeed.value
            return nf.value, nfeed.value
        if d_mpx_ptr is not None or mpx is not None:
            in_fmt = int(fmt) if fmt is not None else FMD_IQ_U8 if u8 else FMD_IQ_F32
            nm = C.c_uint()
            _check(lib().fmd_batch_process_device_mpx(self._h, d_iq_ptr, in_fmt, iq_stride, samples, d_audio_ptr,
                                                      pcm_format_of(pcm), audio_stride, C.byref(nf), d_mpx_ptr,
                                                      mpx_format_of(FMD_MPX_F32 if mpx is None else mpx), mpx_stride,
                                                      C.byref(nm), stream))
            return nf.value, nm.value
        if pcm is not None:
            in_fmt = int(fmt) if fmt is not None else FMD_IQ_U8 if u8 else FMD_IQ_F32
            _check(lib().fmd_batch_process_device_pcm(self._h, d_iq_ptr, in_fmt, iq_stride, samples, d_audio_ptr,
                                                      pcm_format_of(pcm), audio_stride, C.byref(nf), stream))
            return nf.value
        if fmt is not None:
            _check(lib().fmd_batch_process_device_fmt(self._h, d_iq_ptr, int(fmt), iq_stride, samples, d_audio_ptr,
                                                      audio_stride, C.byref(nf), stream))
            return nf.value
        fn = lib().fmd_batch_process_device_u8 if u8 else lib().fmd_batch_process_device
        _check(fn(self._h, d_iq_ptr, iq_stride, samples, d_audio_ptr, audio_stride, C.byref(nf),
                  stream))
        return nf.value

    def pcm_clipped(self):
        """uint64[C]: audio samples (L and R counted separately) that FMD_PCM_S16 calls have saturated since the batch
        was created (fmd_batch_read_pcm_clipped); waits for every call submitted so far."""
        out = np.zeros(self.n_channels, dtype=np.uint64)
        _check(lib().fmd_batch_read_pcm_clipped(self._h, 0, self.n_channels, out.ctypes.data))
        return out

    def set_rds_blocks(self, mode, queue_records=0):
        """The block observation of every call submitted from now on (fmd_batch_set_rds_blocks): 0 off, 1 reception
        counters, 2 counters and a record of every block decision."""
        _check(lib().fmd_batch_set_rds_blocks(self._h, int(mode), int(queue_records)))

    def rds_blocks(self):
        return _check(lib().fmd_batch_get_rds_blocks(self._h))

    def collect_rds_blocks(self, cap=65536, lag=0, stream=None):
        """(records, lost): the block records of the calls at least `lag` old as a structured array (RDS_BLOCK_DTYPE),
        sorted by (call_index, channel, bit_index), and how many were dropped (a full queue, or cap)."""
        buf = np.zeros(max(cap, 1), dtype=RDS_BLOCK_DTYPE)
        lost = C.c_uint(0)
        n = _check(lib().fmd_batch_collect_rds_blocks(self._h, buf.ctypes.data if cap else None, cap, lag, stream,
                                                      C.byref(lost)))
        return buf[:n].copy(), lost.value

    def rds_quality(self, first=0, n=None):
        """The reception counters of channels [first, first + n) as a structured array (RDS_QUALITY_DTYPE); waits for
        every call submitted so far."""
        n = self.n_channels - first if n is None else n
        out = np.zeros(max(n, 1), dtype=RDS_QUALITY_DTYPE)
        _check(lib().fmd_batch_read_rds_quality(self._h, first, n, out.ctypes.data))
        return out[:n]

    def set_loudness(self, on, block_frames=0, ring_blocks=0):
        """The loudness meter of every call submitted from now on (fmd_batch_set_loudness): BS.1770 K-weighted block
        sums and sample peaks of every channel.  block_frames 0: 100 ms; ring_blocks 0: 64; both are fixed by the first
        call that turns the meter on."""
        _check(lib().fmd_batch_set_loudness(self._h, 1 if on else 0, int(block_frames), int(ring_blocks)))
        if on and not getattr(self, "_loud_ring", 0):
            self._loud_ring = int(ring_blocks) or 64

    def loudness(self):
        return _check(lib().fmd_batch_get_loudness(self._h))

    def loudness_block_frames(self):
        return int(lib().fmd_batch_loudness_block_frames(self._h))

    def loudness_coeffs(self):
        """float32[10]: b0 b1 b2 a1 a2 of the high shelf, then of the high-pass."""
        out = np.zeros(10, dtype=np.float32)
        _check(lib().fmd_batch_get_loudness_coeffs(self._h, out.ctypes.data))
        return out

    def collect_loudness(self, lag=0, channels=None, cap=None, stream=None, with_lost=False):
        """(blocks, first): the not-yet-collected block records completed by calls at least `lag` old as a structured
        array [blocks, channels] (LOUD_BLOCK_DTYPE) and the index of the first (fmd_batch_collect_loudness).  channels:
        (first, n), default every channel.  cap: the most blocks one collect takes, default the ring_blocks given to
        set_loudness (64): what the ring can hold.  with_lost: (blocks, first, lost) -- blocks the ring had
        overwritten.  The staging buffer is kept and grown as needed, not allocated per collect."""
        first_ch, n_ch = (0, self.n_channels) if channels is None else (int(channels[0]), int(channels[1]))
        cap = int(getattr(self, "_loud_ring", 0) or 64) if cap is None else int(cap)
        need = max(cap, 1) * max(n_ch, 1)
        buf = getattr(self, "_loud_buf", None)
        if buf is None or buf.size < need:
            buf = self._loud_buf = np.empty(need, dtype=LOUD_BLOCK_DTYPE)
        first, lost = C.c_uint64(0), C.c_uint(0)
        n = _check(lib().fmd_batch_collect_loudness(self._h, buf.ctypes.data, cap, first_ch, n_ch, lag, stream,
                                                    C.byref(first), C.byref(lost)))
        out = buf[:n * n_ch].reshape(n, n_ch).copy()
        return (out, first.value, lost.value) if with_lost else (out, first.value)

    def debug_loud_skip_carry(self, on):
        """Test aid: drop the block in progress at every call boundary (fmd_batch_debug_loud_skip_carry)."""
        _check(lib().fmd_batch_debug_loud_skip_carry(self._h, int(on)))

    def collect_rds_array(self, cap=65536, run_group_decoder=False, stream=None, lag=0):
        """Queued RDS groups as a numpy structured array (channel, call_index, blocks[4])."""
        if getattr(self, "_rds_buf", None) is None or self._rds_buf.size < cap:
            self._rds_buf = np.zeros(cap, dtype=RDS_GROUP_DTYPE)
        n = _check(lib().fmd_batch_collect_rds_lagged(self._h, self._rds_buf.ctypes.data, cap,
                                                      int(run_group_decoder), lag, stream))
        return self._rds_buf[:n].copy()

    def collect_rds(self, cap=65536, run_group_decoder=False, stream=None, lag=0):
        """Queued RDS groups as a list of (channel, call_index, (b0, b1, b2, b3))."""
        a = self.collect_rds_array(cap, run_group_decoder, stream, lag)
        return [(int(c), int(k), tuple(int(x) for x in b))
                for c, k, b in zip(a["channel"], a["call_index"], a["blocks"])]

    def export_rds_device(self, d_records_ptr, cap, channel_offset=0, stream=None, lag=0):
        """Queued RDS groups of calls at least `lag` old -> [cap, 4] int32 rows in device memory
        (fmd_batch_export_rds_device), asynchronously on `stream`.  True: groups were lost."""
        return _check(lib().fmd_batch_export_rds_device(self._h, d_records_ptr, cap, channel_offset, lag,
                                                        stream)) == FMD_WARN_RDS_LOST

    def streams_sharing_queue(self):
        """Internal streams that share a hardware queue with another stream of the process (0: none)."""
        return lib().fmd_batch_streams_sharing_queue(self._h)

    def set_channels_per_capture(self, k):
        """k consecutive channels tune the same capture; the process calls then take one input row per capture."""
        _check(lib().fmd_batch_set_channels_per_capture(self._h, int(k)))
        self.channels_per_capture = max(1, int(k))

    def set_concurrency(self, mode):
        _check(lib().fmd_batch_set_concurrency(self._h, int(mode)))

    def wait(self, stream=None, lag=0):
        """Returns True when RDS groups were lost since the last report (FMD_WARN_RDS_LOST)."""
        return _check(lib().fmd_batch_wait_lagged(self._h, lag, stream)) == FMD_WARN_RDS_LOST

    def take_rds_lost(self):
        return bool(_check(lib().fmd_batch_take_rds_lost(self._h)))

    def status_call_index(self, channel=0):
        """Index of the call whose status the getters return right now (0 = none yet)."""
        ci = C.c_uint32()
        _check(lib().fmd_batch_status_call_index(self._h, channel, C.byref(ci)))
        return ci.value

    def debug_timeline(self, cap=512):
        """[calls, 10] ms since the first profiled call's FIR start: FIR, serial stage, audio tail,
        half-band chain, resampler (start, end each); empty unless calls overlap at profiling level 1."""
        buf = np.full((cap, 10), -1.0, dtype=np.float32)
        n = _check(lib().fmd_batch_debug_timeline(self._h, buf.ctypes.data, cap))
        return buf[:n].copy()

    def debug_stream_conflicts(self, stream=None):
        """Bit mask of internal streams that share a hardware queue with `stream` (0: none); drains the device."""
        return _check(lib().fmd_batch_debug_stream_conflicts(self._h, stream))

    def debug_set_spin_limit(self, limit):
        _check(lib().fmd_batch_debug_set_spin_limit(self._h, limit))

    def debug_set(self, key, value):
        """Development switch of this batch by name (fmd_batch_debug_set)."""
        _check(lib().fmd_batch_debug_set(self._h, key.encode(), int(value)))

    def debug_mpx_ms(self):
        """ms of the multiplex writer in the last (up to 8) _mpx calls; the first query switches the timing on and
        returns nothing (fmd_batch_debug_mpx_ms)."""
        buf = np.zeros(8, dtype=np.float32)
        n = _check(lib().fmd_batch_debug_mpx_ms(self._h, buf.ctypes.data, buf.size))
        return buf[:n].copy()

    def debug_host_ms(self):
        """(calls, {copy_in, submit, wait_copy_out, rds_callbacks}) mean ms of the host-buffer calls since
        the last query (fmd_batch_debug_host_ms)."""
        out = (C.c_float * 4)()
        n = _check(lib().fmd_batch_debug_host_ms(self._h, out))
        return n, dict(zip(("copy_in", "submit", "wait_copy_out", "rds_callbacks"), (float(v) for v in out)))

    def status(self, channel=0):
        st = FmdStatus()
        _check(lib().fmd_batch_get_status(self._h, channel, C.byref(st)))
        return st

    def audio_level(self, channel=0):
        """(audio_mean, audio_rms, m_AudioLevel) of cRadioReceiver::DemuxRead for one channel."""
        a = FmdAudioLevel()
        _check(lib().fmd_batch_get_audio_level(self._h, channel, C.byref(a)))
        return (a.mean, a.rms, a.level)

    def debug_serial_probe(self):
        """FMD_SERIAL_PROBE=1: (start, end, cycles) int64 per workgroup of the serial stage's last 8
        launches, shape (8, slots, 3), launch = call index mod 8; unused slots are zero."""
        buf = np.zeros((8 * 4096, 3), dtype=np.int64)
        n = _check(lib().fmd_batch_debug_serial_probe(self._h, buf.ctypes.data, buf.shape[0]))
        n -= n % 8
        return buf[:n].reshape(8, -1, 3).copy() if n else buf[:0].reshape(8, 0, 3)

    def tap(self, name, channel=0):
        cap = 2 * 65536
        buf = np.zeros(cap, dtype=np.float32)
        n = _check(lib().fmd_batch_get_tap(self._h, TAPS[name], channel, buf.ctypes.data, cap))
        if name in ("demod", "rds_lpf"):
            return buf[:2 * n].view(np.complex64).copy()
        return buf[:n].copy()

    def enable_taps(self, on=True):
        _check(lib().fmd_batch_set_debug_taps(self._h, int(on)))

    def design(self, name):
        buf = np.zeros(16384, dtype=np.float32)
        n = _check(lib().fmd_batch_get_design(self._h, DESIGN[name], buf.ctypes.data, buf.size))
        return buf[:n].copy()

    def scalars(self):
        return dict(zip(SCALAR_NAMES, self.design("scalars")))

    def set_profiling(self, level=2):
        _check(lib().fmd_batch_set_profiling(self._h, int(level)))

    def stage_ms(self):
        """(average ms per stage, number of calls averaged); stages not covered read -1."""
        buf = np.full(32, -1.0, dtype=np.float32)
        calls = _check(lib().fmd_batch_get_stage_ms(self._h, buf.ctypes.data, buf.size))
        out = {}
        i = 0
        while True:
            name = lib().fmd_stage_name(i).decode()
            if not name:
                break
            out[name] = float(buf[i])
            i += 1
        return out, calls


class _BatchView(Batch):
    """A batch somebody else owns (FmDecoder.batch_view)."""

    def __init__(self, handle, sink):
        self._h = handle
        self.sink = sink
        self.n_channels = 1

    def close(self):
        self._h = None

    def __del__(self):
        pass


class FmDecoder:
    """The reference's cFmDecoder surface (FmDecode.h:110-165) on the GPU library."""

    def __init__(self, sample_rate_if, tuning_offset, sample_rate_pcm, bandwidth_pcm=15000.0,
                 downsample=1, USver=False):
        self.sink = _CallbackSink()
        p = make_params(sample_rate_if, tuning_offset, sample_rate_pcm, bandwidth_pcm, downsample,
                        USver)
        h = C.c_void_p()
        _check(lib().fmd_create(C.byref(p), C.byref(self.sink.struct), None, C.byref(h)))
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            lib().fmd_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()

    def Reset(self):
        _check(lib().fmd_reset(self._h))

    def SaveState(self):
        """The decoder's state as an opaque blob (fmd_save_state); LoadState of it into a decoder created with the
        same arguments continues the stream bit for bit."""
        view = self.batch_view()
        buf = np.empty(lib().fmd_batch_state_size(view._h, 1), dtype=np.uint8)
        n = C.c_size_t()
        _check(lib().fmd_save_state(self._h, buf.ctypes.data, buf.size, C.byref(n)))
        return buf[:n.value].tobytes()

    def LoadState(self, blob):
        buf = np.frombuffer(blob, dtype=np.uint8)
        _check(lib().fmd_load_state(self._h, buf.ctypes.data if buf.size else None, buf.size))

    def batch_view(self):
        """The decoder's one-channel batch as a Batch object that does not own it: for the profiling and
        development calls (set_profiling, stage_ms, debug_host_ms, debug_set), not for processing."""
        return _BatchView(C.c_void_p(lib().fmd_decoder_batch(self._h)), self.sink)

    def ProcessStream(self, samples_in):
        iq = np.ascontiguousarray(samples_in)
        if iq.dtype != np.complex64:
            iq = iq.astype(np.float32).view(np.complex64)
        audio = np.empty(2 * iq.size, dtype=np.float32)  # RadioReceiver.cpp:519-520 sizing
        n = _check(lib().fmd_process_stream(self._h, iq.ctypes.data, iq.size, audio.ctypes.data))
        return audio[:n]

    def ProcessStreamToPcm16(self, samples_in):
        """ProcessStream with the audio as interleaved int16 L, R (FMD_PCM_S16, fmd_process_stream_pcm)."""
        iq = np.ascontiguousarray(samples_in)
        if iq.dtype != np.complex64:
            iq = iq.astype(np.float32).view(np.complex64)
        audio = np.empty(2 * iq.size, dtype=np.int16)
        n = _check(lib().fmd_process_stream_pcm(self._h, iq.ctypes.data, FMD_IQ_F32, iq.size, audio.ctypes.data,
                                                FMD_PCM_S16))
        return audio[:n]

    def ProcessStreamWithMpx(self, samples_in, mpx=np.float32):
        """(ProcessStream's audio, the demodulated multiplex of the block as float32 or int16): FMD_MPX_*,
        fmd_process_stream_mpx."""
        iq = np.ascontiguousarray(samples_in)
        if iq.dtype != np.complex64:
            iq = iq.astype(np.float32).view(np.complex64)
        mpx_fmt = mpx_format_of(mpx)
        audio = np.empty(2 * iq.size, dtype=np.float32)
        rows = np.empty(iq.size, dtype=np.int16 if mpx_fmt == FMD_MPX_S16 else np.float32)
        nm = C.c_uint()
        n = _check(lib().fmd_process_stream_mpx(self._h, iq.ctypes.data, FMD_IQ_F32, iq.size, audio.ctypes.data,
                                                FMD_PCM_F32, rows.ctypes.data, mpx_fmt, C.byref(nm)))
        return audio[:n], rows[:nm.value]

    def SetFeed(self, divisor):
        """Turn the decoder's mono feed at sample_rate_pcm / divisor on (2 or 3) or off (0): fmd_batch_set_feed on
        the batch behind the decoder."""
        _check(lib().fmd_batch_set_feed(lib().fmd_decoder_batch(self._h), int(divisor)))

    def ProcessStreamWithFeed(self, samples_in, feed=np.int16):
        """(ProcessStream's audio, the mono feed of the block as int16 or float32): FMD_FEED_*,
        fmd_process_stream_feed; SetFeed first."""
        iq = np.ascontiguousarray(samples_in)
        if iq.dtype != np.complex64:
            iq = iq.astype(np.float32).view(np.complex64)
        feed_fmt = feed_format_of(feed)
        audio = np.empty(2 * iq.size, dtype=np.float32)
        rows = np.empty(iq.size, dtype=np.int16 if feed_fmt == FMD_FEED_S16 else np.float32)
        nfeed = C.c_uint()
        n = _check(lib().fmd_process_stream_feed(self._h, iq.ctypes.data, FMD_IQ_F32, iq.size, audio.ctypes.data,
                                                 FMD_PCM_F32, rows.ctypes.data, feed_fmt, C.byref(nfeed)))
        return audio[:n], rows[:nfeed.value]

    def ProcessStreamWithChannelIq(self, samples_in, ciq=np.complex64):
        """(ProcessStream's audio, the block's IF-filtered IQ as complex64 [M] or int16 [M, 2]): FMD_CIQ_*,
        fmd_process_stream_call."""
        iq = np.ascontiguousarray(samples_in)
        if iq.dtype != np.complex64:
            iq = iq.astype(np.float32).view(np.complex64)
        ciq_fmt = ciq_format_of(ciq)
        audio = np.empty(2 * iq.size, dtype=np.float32)
        rows = _ciq_rows(ciq_fmt, 1, iq.size)[0]
        nq = C.c_uint()
        call = make_call(iq.ctypes.data, FMD_IQ_F32, 0, iq.size, audio=make_rows(audio.ctypes.data, FMD_PCM_F32),
                         ciq=make_rows(rows.ctypes.data, ciq_fmt, 0, nq))
        n = _check(lib().fmd_process_stream_call(self._h, C.byref(call)))
        return audio[:n], rows[:nq.value]

    def ProcessChannelIq(self, ciq_in, pcm=None, mpx=None):
        """One call from the block's channel IQ, the samples behind the IF stage (FMD_IN_CIQ_*, fmd_process_stream_call):
        ciq_in is complex64 [M] or int16 [M, 2] by dtype.  The audio (pcm=np.int16: FMD_PCM_S16); with mpx=np.float32 /
        np.int16 also the multiplex, as ProcessStreamWithMpx returns it."""
        ptr, fmt, _, m = ciq_in_of(ciq_in)
        pcm_fmt = pcm_format_of(pcm)
        # (the largest block's bound: it holds for every baseband length a call may have)
        audio = np.empty(lib().fmd_batch_max_audio_floats(lib().fmd_decoder_batch(self._h), 65536),
                         dtype=np.int16 if pcm_fmt == FMD_PCM_S16 else np.float32)
        call = make_call(ptr, fmt, 0, m, audio=make_rows(audio.ctypes.data, pcm_fmt))
        nm = C.c_uint()
        if mpx is not None:
            mpx_fmt = mpx_format_of(mpx)
            rows = np.empty(max(m, 1), dtype=np.int16 if mpx_fmt == FMD_MPX_S16 else np.float32)
            call.mpx = make_rows(rows.ctypes.data, mpx_fmt, 0, nm)
        n = _check(lib().fmd_process_stream_call(self._h, C.byref(call)))
        return audio[:n] if mpx is None else (audio[:n], rows[:nm.value])

    def ProcessStreamU8(self, buf):
        """ReadAsyncCB + ProcessStream (RTL_SDR_Source.cpp:196-213): buf = I,Q byte pairs."""
        buf = np.ascontiguousarray(buf, dtype=np.uint8)
        n_iq = buf.size // 2
        audio = np.empty(2 * n_iq, dtype=np.float32)
        n = _check(lib().fmd_process_stream_u8(self._h, buf.ctypes.data, n_iq, audio.ctypes.data))
        return audio[:n]

    def _process_stream_fmt(self, buf, dtype, fmt):
        buf = np.ascontiguousarray(buf, dtype=dtype)
        n_iq = buf.size // 2
        audio = np.empty(2 * n_iq, dtype=np.float32)
        n = _check(lib().fmd_process_stream_fmt(self._h, buf.ctypes.data, fmt, n_iq, audio.ctypes.data))
        return audio[:n]

    def ProcessStreamS8(self, buf):
        """buf = I,Q int8 pairs, v * 2^-7 (HackRF, .cs8): the bits of ProcessStream on the converted block."""
        return self._process_stream_fmt(buf, np.int8, FMD_IQ_S8)

    def ProcessStreamS16(self, buf):
        """buf = I,Q int16 pairs, v * 2^-15 (Airspy, SDRplay, USRP sc16, .cs16)."""
        return self._process_stream_fmt(buf, np.int16, FMD_IQ_S16)

    def _status(self):
        st = FmdStatus()
        _check(lib().fmd_get_status(self._h, C.byref(st)))
        return st

    def StereoDetected(self):
        return bool(self._status().stereo_detected)

    def GetTuningOffset(self):
        return self._status().tuning_offset

    def GetInterfaceLevel(self):
        return self._status().interface_level

    def GetBasebandLevel(self):
        return self._status().baseband_level

    def GetPilotLevel(self):
        return self._status().pilot_level


class GroupDecoder:
    """Host-only UECP group decoder (fmd_group_decoder_*)."""

    def __init__(self):
        self.sink = _CallbackSink()
        self._h = lib().fmd_group_decoder_create(C.byref(self.sink.struct), None, 0)

    def push(self, blocks):
        b = (C.c_uint16 * 4)(*blocks)
        lib().fmd_group_decoder_push(self._h, b)

    def reset(self):
        lib().fmd_group_decoder_reset(self._h)

    @property
    def frames(self):
        return self.sink.frames.get(0, [])

    @property
    def name(self):
        return self.sink.names.get(0, "")

    def __del__(self):
        if getattr(self, "_h", None):
            lib().fmd_group_decoder_destroy(self._h)
            self._h = None


def stuff_uecp_frame(frame):
    out = (C.c_uint8 * (2 * len(frame) + 2))()
    src = (C.c_uint8 * len(frame))(*frame)
    n = lib().fmd_uecp_stuff_frame(src, len(frame), out, len(out))
    return bytes(out[:n])


class Receiver:
    """The stream members of cRadioReceiver around the GPU decoder: WriteDataBuffer,
    EndDataBuffer, DemuxRead, GetSignalStatus (RadioReceiver.cpp:296-349, 387-582)."""

    def __init__(self, sample_rate_if, tuning_offset, downsample, tuner_freq=100.0e6,
                 adapter_name="Generic RTL2832U"):
        p = make_params(sample_rate_if, tuning_offset, 48000.0, 15000.0, downsample)
        h = C.c_void_p()
        _check(lib().fmd_receiver_open(C.byref(p), tuner_freq, adapter_name.encode(), C.byref(h)))
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            lib().fmd_receiver_close(self._h)
            self._h = None

    def __del__(self):
        self.close()

    def write_iq(self, iq):
        iq = np.ascontiguousarray(iq)
        if iq.dtype != np.complex64:
            iq = iq.astype(np.float32).view(np.complex64)
        _check(lib().fmd_receiver_write_iq(self._h, iq.ctypes.data, iq.size))

    def write_u8(self, buf):
        buf = np.ascontiguousarray(buf, dtype=np.uint8)
        _check(lib().fmd_receiver_write_u8(self._h, buf.ctypes.data, buf.size // 2))

    def write(self, buf):
        """One block in the format of its dtype (complex64, or float32 / uint8 / int8 / int16 I, Q pairs): a queued
        block carries its format (fmd_receiver_write_fmt)."""
        buf, fmt, per = iq_format_of(buf)
        _check(lib().fmd_receiver_write_fmt(self._h, buf.ctypes.data, fmt, buf.size // per))

    def end(self):
        lib().fmd_receiver_end(self._h)

    def queued_samples(self):
        return int(lib().fmd_receiver_queued_samples(self._h))

    def set_stream_change(self):
        lib().fmd_receiver_set_stream_change(self._h)

    def demux_read(self):
        """(stream_id, pts, duration, payload bytes) or None (the reference's nullptr)."""
        pkt = FmdDemuxPacket()
        rc = _check(lib().fmd_receiver_demux_read(self._h, C.byref(pkt)))
        if rc == 0:
            return None
        data = bytes(C.string_at(pkt.data, pkt.size)) if pkt.size else b""
        return (pkt.stream_id, pkt.pts, pkt.duration, data)

    def signal_status(self):
        a, b, s = C.c_float(), C.c_float(), C.c_int()
        rc = _check(lib().fmd_receiver_signal_status(self._h, C.byref(a), C.byref(b), C.byref(s)))
        return (a.value, b.value, bool(s.value)) if rc else None

    def pvr_signal_status(self):
        st = FmdPvrSignalStatus()
        rc = _check(lib().fmd_receiver_pvr_signal_status(self._h, C.byref(st)))
        if not rc:
            return None
        return {"adapter_name": st.adapter_name.decode(), "adapter_status": st.adapter_status.decode(),
                "provider_name": st.provider_name.decode("latin-1"), "signal": st.signal,
                "snr": st.snr}


# ---- filter design on the host (no GPU needed), same constructors as the reference ----------
def design_lanczos(order, cutoff):
    """cDownsampleFilter's Lanczos table (DownConvert.cpp:18-56, :78): order + 2 floats."""
    buf = np.zeros(order + 2, np.float32)
    _check(lib().fmd_design_lanczos(order, cutoff, buf.ctypes.data, buf.size))
    return buf


def design_lp_kaiser(scale, astop, fpass, fstop, fs):
    """cFirFilter::InitLPFilter (FirFilter.cpp:44-140)."""
    buf = np.zeros(4096, np.float32)
    n = _check(lib().fmd_design_lp_kaiser(scale, astop, fpass, fstop, fs, buf.ctypes.data, buf.size))
    return buf[:n].copy()


def design_biquad(ftype, f0, q, fs):
    """cIirFilter::Init (IirFilter.cpp:11-60): b0 b1 b2 a1 a2; ftype 0 LP, 1 HP, 2 BP, 3 BR."""
    buf = np.zeros(5, np.float32)
    _check(lib().fmd_design_biquad(ftype, f0, q, fs, buf.ctypes.data))
    return buf


def design_tuner_lut(table_size, freq_shift):
    """cFineTuner's table (FmDecode.cpp:45-58), interleaved re, im."""
    buf = np.zeros(2 * table_size, np.float32)
    _check(lib().fmd_design_tuner_lut(table_size, freq_shift, buf.ctypes.data, buf.size))
    return buf


def debug_math(what, a, b=None):
    """Device build of one csrc/fmd_math.h helper on arrays (see fmd_debug_math)."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    o0, o1 = np.empty_like(a), np.empty_like(a)
    bp = None
    if b is not None:
        b = np.ascontiguousarray(b, dtype=np.float32)
        bp = b.ctypes.data
    _check(lib().fmd_debug_math(what, a.size, a.ctypes.data, bp, o0.ctypes.data, o1.ctypes.data))
    return o0, o1
