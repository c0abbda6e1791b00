"""ctypes binding of libsoftspoken_hip.so (C ABI: include/softspoken.h).

There is no CPU fallback: if the library is missing or there is no gfx950 device, the calls
raise.  ctypes releases the GIL for the duration of every foreign call, so the reference's worker
thread (root/code/backend/worker.py, run from a QThreadPool, silencer_ui.py:243) does not block
the GUI thread while the device works.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# SOFTSPOKEN_LIB: another build of the same library (tests: the -DSS_JITTER build); never a different implementation
LIB_PATH = os.environ.get("SOFTSPOKEN_LIB") or os.path.join(_HERE, "libsoftspoken_hip.so")

SS_OK = 0
SS_ERR_ARG = 1
SS_ERR_HIP = 2
SS_ERR_FORMAT = 3
SS_ERR_STATE = 4
SS_ERR_STOPPED = 5
SS_ERR_NOMEM = 6
SS_ERR_CAPACITY = 7
SS_ERR_RANGE = 8          # f16x2: a weight or an activation has no f16 representation -> run the checkpoint in the fp32 mode
ABI_VERSION = 3
FLAG_BF16 = 1
FLAG_PROFILE = 2
FLAG_F16X2 = 4
PRECISIONS = ("fp32", "f16x2", "bf16")
PCM_U8, PCM_S16, PCM_S24, PCM_S32, PCM_F32, PCM_F64 = 1, 2, 3, 4, 5, 6
PCM_S8, PCM_S16BE, PCM_S24BE, PCM_S32BE, PCM_F32BE, PCM_F64BE = 7, 8, 9, 10, 11, 12    # AIFF / AIFF-C: big endian, 8-bit samples signed

_BPS = {PCM_U8: 1, PCM_S16: 2, PCM_S24: 3, PCM_S32: 4, PCM_F32: 4, PCM_F64: 8,
        PCM_S8: 1, PCM_S16BE: 2, PCM_S24BE: 3, PCM_S32BE: 4, PCM_F32BE: 4, PCM_F64BE: 8}     # bytes per sample of enum ss_pcm_format
SAMPLE_RATE = 22050
WINDOW_SAMPLES = 66150
STEP_SAMPLES = 13230              # floor(22050 * 0.6): the default window step (Context.window_step; STEP_MIN <= step <= STEP_MAX)
DEFAULT_STEP = 0.6
STEP_MIN, STEP_MAX = 0.1, 3.0


class WavInfo(C.Structure):
    _fields_ = [("format", C.c_int32), ("channels", C.c_int32), ("sample_rate", C.c_int32), ("bits", C.c_int32),
                ("frames", C.c_int64), ("data_offset", C.c_int64), ("data_bytes", C.c_int64)]


class Region(C.Structure):
    _fields_ = [("start", C.c_double), ("end", C.c_double)]


class KernelStat(C.Structure):
    _fields_ = [("name", C.c_char * 128), ("launches", C.c_int64), ("total_ms", C.c_double), ("flops", C.c_double),
                ("bytes", C.c_double), ("issued_flops", C.c_double)]


class StreamInfo(C.Structure):
    _fields_ = [("frames_pushed", C.c_int64), ("frames_staged", C.c_int64), ("windows_run", C.c_int64), ("windows_ready", C.c_int64),
                ("final_until_s", C.c_double), ("closed", C.c_int32), ("finished", C.c_int32), ("state_bytes", C.c_int64)]


class StreamErase(C.Structure):
    _fields_ = [("pad_s", C.c_double), ("min_len_s", C.c_double)]


class StreamOutputInfo(C.Structure):
    _fields_ = [("frames_out", C.c_int64), ("frames_held", C.c_int64), ("frames_erased", C.c_int64), ("pad_s", C.c_double),
                ("min_len_s", C.c_double)]


class SeparationParams(C.Structure):
    _fields_ = [("fade_s", C.c_double), ("min_gain", C.c_double), ("above_fmax", C.c_int32), ("speech_channel", C.c_int32)]


class SeparationRange(C.Structure):
    _fields_ = [("frame_begin", C.c_int64), ("frame_end", C.c_int64), ("stft_first", C.c_int64), ("stft_last", C.c_int64),
                ("bin_first", C.c_int64), ("bin_last", C.c_int64), ("win_first", C.c_int64), ("win_last", C.c_int64)]


class SeparationPlanInfo(C.Structure):
    _fields_ = [("n_fft", C.c_int32), ("hop", C.c_int32), ("n_windows", C.c_int64), ("n_bins", C.c_int64), ("windows_run", C.c_int64),
                ("n_ranges", C.c_int64), ("cap_ranges", C.c_int64), ("ranges", C.POINTER(SeparationRange))]


class BandParams(C.Structure):
    _fields_ = [("q_low", C.c_double), ("q_high", C.c_double), ("speech_channel", C.c_int32), ("reserved", C.c_int32)]


class RegionBand(C.Structure):
    _fields_ = [("low_hz", C.c_double), ("high_hz", C.c_double), ("peak_hz", C.c_double), ("speech_share", C.c_double),
                ("band_low", C.c_int32), ("band_high", C.c_int32), ("band_peak", C.c_int32), ("n_bins", C.c_int32)]


# struct ss_region_band as a numpy record (48 bytes)
REGION_BAND_DTYPE = np.dtype([("low_hz", "<f8"), ("high_hz", "<f8"), ("peak_hz", "<f8"), ("speech_share", "<f8"),
                              ("band_low", "<i4"), ("band_high", "<i4"), ("band_peak", "<i4"), ("n_bins", "<i4")])



class BoxParams(C.Structure):
    _fields_ = [("fade_s", C.c_double), ("min_gain", C.c_double), ("edge_hz", C.c_double)]


class BoxRange(C.Structure):
    _fields_ = [("frame_begin", C.c_int64), ("frame_end", C.c_int64), ("stft_first", C.c_int64), ("stft_last", C.c_int64)]


class BoxPlanInfo(C.Structure):
    _fields_ = [("n_fft", C.c_int32), ("hop", C.c_int32), ("n_frames", C.c_int64), ("n_ranges", C.c_int64), ("cap_ranges", C.c_int64),
                ("ranges", C.POINTER(BoxRange))]


# struct ss_box as a numpy record (40 bytes): a time range, its frequency band (NaN: no estimate) and the channel it acts on (-1: all)
BOX_DTYPE = np.dtype([("start", "<f8"), ("end", "<f8"), ("low_hz", "<f8"), ("high_hz", "<f8"), ("channel", "<i4"), ("reserved", "<i4")])

ABOVE_FMAX = {"mute": 0, "keep": 1}      # SS_ABOVE_FMAX_MUTE / _KEEP


PROGRESS_FN = C.CFUNCTYPE(None, C.c_void_p, C.c_int64, C.c_int64)

# every symbol include/softspoken.h declares: (restype, argtypes)
_P = C.c_void_p
_SIGS = {
    "ss_abi_version": (C.c_int, []),
    "ss_last_error": (C.c_char_p, [_P]),
    "ss_wav_parse": (C.c_int, [_P, C.c_size_t, C.POINTER(WavInfo)]),
    "ss_resampled_length": (C.c_int64, [C.c_int64, C.c_int]),
    "ss_plan_windows": (C.c_int64, [C.c_double, _P, C.c_int64]),
    "ss_plan_windows_step": (C.c_int64, [C.c_double, C.c_double, _P, C.c_int64]),
    "ss_window_start_bin": (C.c_int64, [C.c_int64, C.c_double]),
    "ss_find_regions": (C.c_int, [_P, _P, C.c_int64, C.c_double, C.c_double, _P, C.c_int64, C.POINTER(C.c_int64)]),
    "ss_find_regions_union": (C.c_int, [_P, _P, C.c_int64, C.c_int, C.c_double, C.c_double, _P, C.c_int64, C.POINTER(C.c_int64)]),
    "ss_format_csv_rows": (C.c_int64, [C.c_char_p, C.c_char_p, _P, C.c_int64, C.c_int64, _P, C.c_int64]),
    "ss_create": (C.c_int, [C.c_int, _P, C.c_size_t, C.c_uint32, C.POINTER(_P)]),
    "ss_destroy": (None, [_P]),
    "ss_set_chunk_windows": (C.c_int, [_P, C.c_int]),
    "ss_set_window_step": (C.c_int, [_P, C.c_double]),
    "ss_get_window_step": (C.c_double, [_P]),
    "ss_reset": (C.c_int, [_P]),
    "ss_reset_generation": (C.c_uint64, [_P]),
    "ss_add_pcm": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int64, C.POINTER(C.c_int)]),
    "ss_add_pcm_device": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int64, C.POINTER(C.c_int)]),
    "ss_add_pcm_batch_device": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, _P, C.c_int, C.POINTER(C.c_int)]),
    "ss_add_pcm_channels": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int64, C.POINTER(C.c_int)]),
    "ss_add_pcm_channels_device": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int64, C.POINTER(C.c_int)]),
    "ss_add_pcm_channels_batch_device": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, _P, C.c_int, C.POINTER(C.c_int)]),
    "ss_add_f32_22k": (C.c_int, [_P, _P, C.c_int64, C.POINTER(C.c_int)]),
    "ss_add_padded_f32_22k": (C.c_int, [_P, _P, C.c_int64, C.POINTER(C.c_int)]),
    "ss_signal_length": (C.c_int64, [_P, C.c_int, C.c_int]),
    "ss_read_signal": (C.c_int, [_P, C.c_int, C.c_int, C.c_int64, C.c_int64, _P]),
    "ss_silence_pcm": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int64, _P, C.c_int64, _P]),
    "ss_wav_header_pcm16": (C.c_int, [C.c_int, C.c_int, C.c_int64, _P]),
    "ss_stft512_frames": (C.c_int64, [C.c_int64]),
    "ss_stft512_magnitude": (C.c_int, [_P, _P, C.c_int64, _P, C.c_int64]),
    "ss_device_alloc": (C.c_int, [_P, C.c_size_t, C.POINTER(_P)]),
    "ss_device_free": (C.c_int, [_P, _P]),
    "ss_device_upload": (C.c_int, [_P, _P, _P, C.c_size_t]),
    "ss_host_alloc": (C.c_int, [_P, C.c_size_t, C.POINTER(_P)]),
    "ss_host_free": (C.c_int, [_P, _P]),
    "ss_upload_wav_batch_async": (C.c_int, [_P, _P, _P, C.c_int, _P, C.c_size_t, _P]),
    "ss_device_upload_async": (C.c_int, [_P, _P, _P, C.c_size_t]),
    "ss_upload_wait": (C.c_int, [_P]),
    "ss_features": (C.c_int, [_P, C.c_int, _P, C.c_int, _P]),
    "ss_infer_windows": (C.c_int, [_P, C.c_int, _P, C.c_int, _P, _P]),
    "ss_run": (C.c_int, [_P, C.c_double, C.c_double, _P, _P, _P]),
    "ss_run_begin": (C.c_int, [_P, C.c_double, C.c_double]),
    "ss_run_end": (C.c_int, [_P]),
    "ss_run_begin_tracked": (C.c_int, [_P, C.c_double, C.c_double]),
    "ss_run_poll": (C.c_int, [_P, _P, _P, C.c_int]),
    "ss_run_from_logits": (C.c_int, [_P, _P, C.c_int64, C.c_double, C.c_double]),
    "ss_num_windows": (C.c_int64, [_P, C.c_int]),
    "ss_get_window_logits": (C.c_int, [_P, C.c_int, _P, C.c_int64]),
    "ss_get_avg": (C.c_int, [_P, C.c_int, _P, _P, C.c_int64, C.POINTER(C.c_int64)]),
    "ss_get_regions": (C.c_int, [_P, C.c_int, _P, C.c_int64, C.POINTER(C.c_int64)]),
    "ss_get_regions_batch": (C.c_int, [_P, C.c_int, C.c_int, _P, _P, C.c_int64, C.POINTER(C.c_int64)]),
    "ss_get_regions_union": (C.c_int, [_P, C.c_int, C.c_int, _P, C.c_int64, C.POINTER(C.c_int64)]),
    "ss_get_region_peaks": (C.c_int, [_P, C.c_int, C.c_int, _P, C.c_int64, C.POINTER(C.c_int64)]),
    "ss_sync": (C.c_int, [_P]),
    "ss_reset_kernel_stats": (C.c_int, [_P]),
    "ss_get_kernel_stats": (C.c_int, [_P, _P, C.c_int, C.POINTER(C.c_int)]),
    "ss_last_run_device_ms": (C.c_double, [_P]),
    "ss_workspace_bytes": (C.c_int64, [_P]),
    "ss_stream_open": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.POINTER(C.c_int)]),
    "ss_stream_push": (C.c_int, [_P, C.c_int, _P, C.c_int64]),
    "ss_stream_close": (C.c_int, [_P, C.c_int]),
    "ss_stream_step": (C.c_int, [_P]),
    "ss_stream_regions": (C.c_int, [_P, C.c_int, _P, C.c_int64, C.POINTER(C.c_int64)]),
    "ss_stream_avg": (C.c_int, [_P, C.c_int, _P, _P, C.c_int64, C.POINTER(C.c_int64)]),
    "ss_stream_get_info": (C.c_int, [_P, C.c_int, C.POINTER(StreamInfo)]),
    "ss_stream_free": (C.c_int, [_P, C.c_int]),
    "ss_stream_export": (C.c_int, [_P, C.c_int, _P, C.c_int64, C.POINTER(C.c_int64)]),
    "ss_stream_import": (C.c_int, [_P, _P, C.c_int64, C.POINTER(C.c_int)]),
    "ss_erase_table": (C.c_int, [_P, C.c_int64, C.POINTER(StreamErase), _P, C.c_int64, C.POINTER(C.c_int64)]),
    "ss_stream_output_limit": (C.c_int64, [C.c_int, C.c_int64, C.c_int, C.c_double, C.c_double, C.POINTER(StreamErase)]),
    "ss_stream_open_output": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.POINTER(StreamErase), C.POINTER(C.c_int)]),
    "ss_stream_output": (C.c_int, [_P, C.c_int, _P, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "ss_stream_get_output_info": (C.c_int, [_P, C.c_int, C.POINTER(StreamOutputInfo)]),
    "ss_stream_open_channels": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.POINTER(StreamErase), C.c_int, C.POINTER(C.c_int)]),
    "ss_stream_open_source": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.POINTER(StreamErase), C.c_int, C.POINTER(C.c_int)]),
    "ss_stream_output_bytes": (C.c_int, [_P, C.c_int, _P, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "ss_stream_avg_channel": (C.c_int, [_P, C.c_int, C.c_int, _P, _P, C.c_int64, C.POINTER(C.c_int64)]),
    "ss_stream_region_peaks": (C.c_int, [_P, C.c_int, _P, C.c_int64, C.POINTER(C.c_int64)]),
    "ss_stream_open_bands": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.POINTER(StreamErase), C.c_int, C.c_int,
                                       C.POINTER(BandParams), C.c_int, C.POINTER(C.c_int)]),
    "ss_stream_bands": (C.c_int, [_P, C.c_int, _P, _P, C.c_int64, C.POINTER(C.c_int64)]),
    "ss_stream_separate_limit": (C.c_int64, [C.c_int, C.c_int64, C.c_int64, C.c_int, C.c_double, C.c_double, C.POINTER(StreamErase),
                                             C.POINTER(SeparationParams)]),
    "ss_stream_separate_latency": (C.c_double, [C.c_int, C.c_double, C.POINTER(StreamErase), C.POINTER(SeparationParams)]),
    "ss_separation_plan": (C.c_int, [C.c_int, C.c_int64, _P, C.c_int64, C.POINTER(SeparationParams), C.POINTER(SeparationPlanInfo)]),
    "ss_separation_maps": (C.c_int, [_P, C.c_int, C.c_int64, C.c_int64, _P]),
    "ss_separate_pcm": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int64, _P, C.c_int64, C.POINTER(SeparationParams), _P]),
    "ss_separate_pcm_channels": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int64, _P, C.c_int64, C.POINTER(SeparationParams), _P]),
    "ss_silence_pcm_source": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int64, _P, C.c_int64, _P, C.c_int64]),
    "ss_separate_pcm_source": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int64, _P, C.c_int64, C.POINTER(SeparationParams), _P,
                                         C.c_int64]),
    "ss_separate_pcm_channels_source": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int64, _P, C.c_int64,
                                                  C.POINTER(SeparationParams), _P, C.c_int64]),
    "ss_wav_header": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int64, _P]),
    "ss_box_plan": (C.c_int, [C.c_int, C.c_int64, _P, C.c_int64, C.POINTER(BoxParams), C.POINTER(BoxPlanInfo)]),
    "ss_box_silence_pcm": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int64, _P, C.c_int64, C.POINTER(BoxParams), _P]),
    "ss_box_silence_pcm_source": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int64, _P, C.c_int64, C.POINTER(BoxParams), _P, C.c_int64]),
    "ss_band_edges": (C.c_int, [_P]),
    "ss_region_bins": (C.c_int, [C.c_double, C.c_double, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "ss_region_bands": (C.c_int, [_P, C.c_int, C.c_int, _P, C.c_int64, C.POINTER(BandParams), _P, _P]),
    "ss_region_bands_from_maps": (C.c_int, [_P, _P, C.c_int, C.c_int64, C.c_int64, _P, C.c_int64, C.POINTER(BandParams), _P, _P]),
}
EXPORTS = tuple(_SIGS)
# exported by the development build only (libsoftspoken_hip_dev.so, loaded through SOFTSPOKEN_LIB by tests and tools)
_DEV_SIGS = {
    "ss_debug_fail_workspace_alloc": (C.c_int, [_P, C.c_int]),
    "ss_debug_set_separation_budget": (C.c_int, [_P, C.c_int64]),
    "ss_debug_set_bands_budget": (C.c_int, [_P, C.c_int64]),
    "ss_debug_activation": (C.c_int, [_P, C.c_char_p, C.c_int, C.c_int64, C.c_int64, _P, C.c_int64, _P, _P]),
}

_lib = None


class NativeError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"libsoftspoken_hip: status {code}: {msg}")
        self.code = code


def lib():
    """Load the shared library (once).  Raises if it has not been built: no fallback."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"{LIB_PATH} not found - build it with `python -m softspoken_amd.build` "
                              "(the voice-detector path has no CPU fallback)")
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in _SIGS.items():
            fn = getattr(L, name)
            fn.restype, fn.argtypes = res, args
        for name, (res, args) in _DEV_SIGS.items():
            fn = getattr(L, name, None)
            if fn is not None:
                fn.restype, fn.argtypes = res, args
        if L.ss_abi_version() != ABI_VERSION:
            raise ImportError(f"{LIB_PATH}: ABI version {L.ss_abi_version()}, this binding is for {ABI_VERSION} -- a stale build "
                              "(python -m softspoken_amd.build --force)")
        _lib = L
    return _lib


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _check(rc, ctx=None):
    if rc != SS_OK:
        msg = lib().ss_last_error(ctx)
        raise NativeError(rc, msg.decode("utf-8", "replace") if msg else "")


# ---- host-only helpers ----------------------------------------------------------------------------
def wav_parse(buf) -> WavInfo:
    a = np.frombuffer(buf, dtype=np.uint8)
    info = WavInfo()
    _check(lib().ss_wav_parse(_ptr(a), a.size, C.byref(info)))
    return info


def check_step(step) -> float:
    """step as a float, or ValueError naming the limits (the library answers SS_ERR_ARG / -1 for the same values)."""
    try:
        s = float(step)
    except (TypeError, ValueError):
        s = float("nan")
    if not (STEP_MIN <= s <= STEP_MAX):                   # (a NaN compares false)
        raise ValueError(f"window step must be a finite number of seconds in [{STEP_MIN}, {STEP_MAX}], not {step!r}")
    return s


def plan_windows(duration_s: float, step: float = DEFAULT_STEP) -> np.ndarray:
    """Window starts in the 3 s-padded signal: i * floor(22050 * step) (ss_plan_windows_step)."""
    step = check_step(step)
    n = lib().ss_plan_windows_step(float(duration_s), step, None, 0)
    out = np.zeros(max(n, 0), dtype=np.int64)
    if n > 0:
        lib().ss_plan_windows_step(float(duration_s), step, _ptr(out), n)
    return out


def window_start_bin(i: int, step: float = DEFAULT_STEP) -> int:
    """First averaged bin of window i: int(round(i * step / (3 / 256))), ties to even (ss_window_start_bin)."""
    return int(lib().ss_window_start_bin(int(i), check_step(step)))


def find_regions(avg, bin_idx, threshold=0.1, break_s=0.5):
    avg = np.ascontiguousarray(avg, dtype=np.float64)
    bin_idx = np.ascontiguousarray(bin_idx, dtype=np.int64)
    cap = len(avg) // 2 + 1
    out = (Region * cap)()
    n = C.c_int64(0)
    _check(lib().ss_find_regions(_ptr(avg), _ptr(bin_idx), len(avg), threshold, break_s, out, cap, C.byref(n)))
    return [(out[i].start, out[i].end) for i in range(n.value)]


def find_regions_union(avg, bin_idx, threshold=0.1, break_s=0.5):
    """The merged table of a recording's channels ("speech on any channel"): avg [n_channels, n] over one bin_idx [n]."""
    avg = np.ascontiguousarray(avg, dtype=np.float64)
    if avg.ndim != 2:
        raise ValueError("avg must be [n_channels, n]")
    bin_idx = np.ascontiguousarray(bin_idx, dtype=np.int64)
    if bin_idx.shape != (avg.shape[1],):
        raise ValueError("bin_idx must hold one bin number per column of avg")
    cap = avg.shape[1] // 2 + 1
    out = (Region * cap)()
    n = C.c_int64(0)
    _check(lib().ss_find_regions_union(_ptr(avg), _ptr(bin_idx), avg.shape[1], avg.shape[0], threshold, break_s, out, cap, C.byref(n)))
    return [(out[i].start, out[i].end) for i in range(n.value)]


def format_csv_rows(file_path: str, file_name: str, regions, first_id: int = 1) -> str:
    arr = (Region * max(1, len(regions)))()
    for i, (s, e) in enumerate(regions):
        arr[i].start, arr[i].end = float(s), float(e)
    fp, fn = file_path.encode(), file_name.encode()
    need = lib().ss_format_csv_rows(fp, fn, arr, len(regions), first_id, None, 0)
    buf = C.create_string_buffer(need + 1)
    lib().ss_format_csv_rows(fp, fn, arr, len(regions), first_id, buf, need + 1)
    return buf.value.decode()


def wav_header_pcm16(sr: int, channels: int, frames: int) -> bytes:
    buf = C.create_string_buffer(44)
    _check(lib().ss_wav_header_pcm16(int(sr), int(channels), int(frames), buf))
    return buf.raw


def wav_header(fmt: int, sr: int, channels: int, frames: int) -> bytes:
    """The 44-byte RIFF/WAVE header of a file in one of the little-endian encodings 1-6 (ss_wav_header)."""
    buf = C.create_string_buffer(44)
    _check(lib().ss_wav_header(int(fmt), int(sr), int(channels), int(frames), buf))
    return buf.raw


def _regions(regions):
    arr = (Region * max(1, len(regions)))()
    for i, (s, e) in enumerate(regions):
        arr[i].start, arr[i].end = float(s), float(e)
    return arr


def _erase(erase):
    """None, a dict(pad_s=, min_len_s=) or a (pad_s, min_len_s) pair -> struct ss_stream_erase (None: 0, 0)."""
    if erase is None:
        return StreamErase(0.0, 0.0)
    if isinstance(erase, dict):
        unknown = set(erase) - {"pad_s", "min_len_s"}
        if unknown:
            raise ValueError(f"erase: unknown keys {sorted(unknown)}")
        return StreamErase(float(erase.get("pad_s", 0.0)), float(erase.get("min_len_s", 0.0)))
    pad_s, min_len_s = erase
    return StreamErase(float(pad_s), float(min_len_s))


def erase_table(regions, pad_s: float = 0.0, min_len_s: float = 0.0):
    """E(R) of include/softspoken.h (ss_erase_table, host only): regions of end - start <= min_len_s dropped, the others padded."""
    arr = _regions(regions)
    e = StreamErase(float(pad_s), float(min_len_s))
    out = (Region * max(1, len(regions)))()
    n = C.c_int64(0)
    _check(lib().ss_erase_table(arr, len(regions), C.byref(e), out, len(regions), C.byref(n)))
    return [(out[i].start, out[i].end) for i in range(n.value)]


def stream_output_limit(sr: int, bins_final: int, pending=None, pad_s: float = 0.0, min_len_s: float = 0.0) -> int:
    """The frame up to which a stream's output is decided (ss_stream_output_limit, host only), before the clamp to the frames
    decoded.  pending: None, or the (start, end) bin times of the merged candidate that is not final yet, before the -3 s."""
    e = StreamErase(float(pad_s), float(min_len_s))
    ps, pe = pending if pending is not None else (0.0, 0.0)
    v = lib().ss_stream_output_limit(int(sr), int(bins_final), int(pending is not None), float(ps), float(pe), C.byref(e))
    if v == -2 ** 63:
        raise ValueError("ss_stream_output_limit: bad argument")
    return int(v)


def separation_params(fade_s: float = 0.01, min_gain: float = 0.0, above_fmax="mute", speech_channel: int = 1) -> SeparationParams:
    """struct ss_separation_params; above_fmax: "mute" / "keep" (or the SS_ABOVE_FMAX_* code itself: unknown codes reach the library)."""
    code = ABOVE_FMAX[above_fmax] if isinstance(above_fmax, str) else int(above_fmax)
    return SeparationParams(float(fade_s), float(min_gain), code, int(speech_channel))


def stream_separate_limit(sr: int, frames_decoded: int, bins_final: int, pending=None, pad_s: float = 0.0, min_len_s: float = 0.0, **params) -> int:
    """The frame up to which a separation stream's output would be decided (ss_stream_separate_limit, host only), before the clamp to
    [frames_out, frames decoded].  pending as stream_output_limit's; params: separation_params' keywords."""
    e = StreamErase(float(pad_s), float(min_len_s))
    p = separation_params(**params)
    ps, pe = pending if pending is not None else (0.0, 0.0)
    v = lib().ss_stream_separate_limit(int(sr), int(frames_decoded), int(bins_final), int(pending is not None), float(ps), float(pe), C.byref(e), C.byref(p))
    if v == -2 ** 63:
        raise ValueError("ss_stream_separate_limit: bad argument")
    return int(v)


def stream_separate_latency(sr: int, break_s: float, pad_s: float = 0.0, min_len_s: float = 0.0, **params) -> float:
    """D_sep in seconds (ss_stream_separate_latency, host only): the most audio a frame returned under that rule lags behind."""
    e = StreamErase(float(pad_s), float(min_len_s))
    p = separation_params(**params)
    v = lib().ss_stream_separate_latency(int(sr), float(break_s), C.byref(e), C.byref(p))
    if v != v:
        raise ValueError("ss_stream_separate_latency: bad argument")
    return float(v)


def separation_plan(sr: int, frames: int, regions, **params) -> dict:
    """ss_separation_plan (host only): n_fft, hop, n_windows, n_bins, windows_run and the merged ranges as a list of dicts."""
    arr = _regions(regions)
    p = separation_params(**params)
    cap = max(1, len(regions))
    rng = (SeparationRange * cap)()
    info = SeparationPlanInfo()
    info.cap_ranges, info.ranges = cap, C.cast(rng, C.POINTER(SeparationRange))
    _check(lib().ss_separation_plan(int(sr), int(frames), arr, len(regions), C.byref(p), C.byref(info)))
    out = {k: int(getattr(info, k)) for k in ("n_fft", "hop", "n_windows", "n_bins", "windows_run")}
    out["ranges"] = [{f: int(getattr(rng[i], f)) for f, _ in SeparationRange._fields_} for i in range(info.n_ranges)]
    return out


def boxes_array(boxes) -> np.ndarray:
    """A BOX_DTYPE array from one, or from rows (start_s, end_s, low_hz, high_hz[, channel]): None or NaN edges mean "no estimate" (the
    whole band), a missing or None channel every channel (-1)."""
    if isinstance(boxes, np.ndarray) and boxes.dtype == BOX_DTYPE:
        return np.ascontiguousarray(boxes)
    out = np.zeros(len(boxes), dtype=BOX_DTYPE)
    for i, b in enumerate(boxes):
        s, e, lo, hi = b[:4]
        ch = b[4] if len(b) > 4 else None
        out[i] = (float(s), float(e), float("nan") if lo is None else float(lo), float("nan") if hi is None else float(hi),
                  -1 if ch is None else int(ch), 0)
    return out


def box_plan(sr: int, frames: int, boxes, fade_s: float = 0.01, min_gain: float = 0.0, edge_hz: float = 100.0) -> dict:
    """ss_box_plan (host only): n_fft, hop, n_frames and the merged ranges (frame_begin, frame_end, stft_first, stft_last) as dicts."""
    arr = boxes_array(boxes)
    p = BoxParams(float(fade_s), float(min_gain), float(edge_hz))
    cap = max(1, len(arr))
    rng = (BoxRange * cap)()
    info = BoxPlanInfo()
    info.cap_ranges, info.ranges = cap, C.cast(rng, C.POINTER(BoxRange))
    _check(lib().ss_box_plan(int(sr), int(frames), _ptr(arr) if len(arr) else None, len(arr), C.byref(p), C.byref(info)))
    out = {k: int(getattr(info, k)) for k in ("n_fft", "hop", "n_frames")}
    out["ranges"] = [{f: int(getattr(rng[i], f)) for f, _ in BoxRange._fields_} for i in range(info.n_ranges)]
    return out


def band_edges() -> np.ndarray:
    """The 130 HTK mel points f of the region bands (ss_band_edges, host only): band m's triangle spans f[m] .. f[m + 2] Hz."""
    out = np.empty(130, dtype=np.float64)
    _check(lib().ss_band_edges(_ptr(out)))
    return out


def region_bins(start: float, end: float, covered_bins: int) -> tuple[int, int]:
    """(first bin, bins) of the region [start, end) s in a file with covered_bins covered bins (ss_region_bins, host only): the bins
    whose centres (j + 0.5) 3 / 256 - 3 s lie inside."""
    first, count = C.c_int64(0), C.c_int64(0)
    _check(lib().ss_region_bins(float(start), float(end), int(covered_bins), C.byref(first), C.byref(count)))
    return first.value, count.value


def band_params(q_low: float = 0.05, q_high: float = 0.95, speech_channel: int = 1) -> BandParams:
    return BandParams(float(q_low), float(q_high), int(speech_channel), 0)


def _band_call(fn, ctx, head, regions, n_sig, q_low, q_high, speech_channel, profile):
    """The tail shared by ss_region_bands and ss_region_bands_from_maps: (bands [n, n_sig] records, profile [n, n_sig, 2, 128] or None)."""
    n = len(regions)
    p = band_params(q_low, q_high, speech_channel)
    out = np.zeros((n, n_sig), dtype=REGION_BAND_DTYPE)
    prof = np.zeros((n, n_sig, 2, 128), dtype=np.float64) if profile else None
    _check(fn(ctx, *head, _regions(regions), n, C.byref(p), _ptr(out) if n else None, _ptr(prof) if profile and n else None), ctx)
    return out, prof


# ---- context --------------------------------------------------------------------------------------
class Context:
    """One detector context on one GPU (not thread-safe; one per device)."""

    def __init__(self, blob: bytes | np.ndarray | None, device: int = 0, bf16: bool = False, profile: bool = False,
                 chunk: int | None = None, precision: str | None = None):
        """blob None -> audio-only context (decode / mixdown / resample; model calls raise).
        precision: "fp32" (fp32 matrix instructions, exact fp32 FMA chains), "f16x2" (fp32-accurate on the f16 matrix cores: operands
        split into two f16 halves, three products per term) or "bf16" (throughput mode, scores differ by up to ~0.1); bf16=True is
        the older spelling of precision="bf16"."""
        L = lib()
        b = np.frombuffer(blob, dtype=np.uint8) if blob is not None else None
        self._h = C.c_void_p()
        precision = precision or ("bf16" if bf16 else "fp32")
        if precision not in PRECISIONS:
            raise ValueError(f"precision must be one of {PRECISIONS}, not {precision!r}")
        bf16 = precision == "bf16"
        self.precision = precision
        flags = (FLAG_BF16 if bf16 else 0) | (FLAG_F16X2 if precision == "f16x2" else 0) | (FLAG_PROFILE if profile else 0)
        rc = L.ss_create(int(device), _ptr(b), b.size if b is not None else 0, flags, C.byref(self._h))
        if rc != SS_OK:
            self._h = C.c_void_p()
            _check(rc)
        self.bf16 = bf16
        self._cb_keep = None
        if chunk:
            self.set_chunk(chunk)

    @property
    def alive(self) -> bool:
        """False once close() has destroyed the native context."""
        return bool(getattr(self, "_h", None) and self._h.value)

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            lib().ss_destroy(self._h)
            self._h = C.c_void_p()

    __del__ = close

    def _ck(self, rc):
        _check(rc, self._h)

    def set_chunk(self, n):
        self._ck(lib().ss_set_chunk_windows(self._h, int(n)))

    def set_window_step(self, step: float):
        """settings.step_size of the reference: seconds between window starts, STEP_MIN <= step <= STEP_MAX (ValueError otherwise).
        Holds for the next run / run_begin / run_from_logits and for streams opened afterwards; not while a run is in flight."""
        self._ck(lib().ss_set_window_step(self._h, check_step(step)))

    @property
    def window_step(self) -> float:
        return float(lib().ss_get_window_step(self._h))

    def reset(self):
        self._ck(lib().ss_reset(self._h))

    def reset_generation(self) -> int:
        """Number of reset() calls so far: file ids handed out before the last one no longer name the caller's files."""
        return int(lib().ss_reset_generation(self._h))

    @staticmethod
    def _need_bytes(pcm: np.ndarray, fmt: int, channels: int, frames) -> None:
        """The C ABI copies frames * channels * bytes_per_sample from the pointer: refuse a shorter buffer here (ValueError),
        where the library would read past its end."""
        if fmt not in _BPS:
            raise ValueError(f"unknown PCM format code {fmt}")
        need = int(np.sum(np.asarray(frames, dtype=np.int64))) * int(channels) * _BPS[fmt]
        if int(channels) < 1 or need < 0 or pcm.nbytes < need:
            raise ValueError(f"PCM buffer holds {pcm.nbytes} bytes, {need} needed for {frames} frames x {channels} channels")

    def add_pcm(self, pcm: np.ndarray, fmt: int, sr: int, channels: int, frames: int) -> int:
        pcm = np.ascontiguousarray(pcm)
        self._need_bytes(pcm, fmt, channels, frames)
        fid = C.c_int(-1)
        self._ck(lib().ss_add_pcm(self._h, _ptr(pcm), fmt, sr, channels, frames, C.byref(fid)))
        return fid.value

    def silence_pcm(self, pcm: np.ndarray, fmt: int, sr: int, channels: int, frames: int, regions) -> np.ndarray:
        """Interleaved int16 (frames, channels) with the (start_s, end_s) regions zeroed."""
        pcm = np.ascontiguousarray(pcm)
        self._need_bytes(pcm, fmt, channels, frames)
        arr = (Region * max(1, len(regions)))()
        for i, (s, e) in enumerate(regions):
            arr[i].start, arr[i].end = float(s), float(e)
        out = np.empty((frames, channels), dtype=np.int16)
        self._ck(lib().ss_silence_pcm(self._h, _ptr(pcm), fmt, sr, channels, frames, arr, len(regions), _ptr(out)))
        return out

    def separate_pcm(self, pcm: np.ndarray, fmt: int, sr: int, channels: int, frames: int, regions, fade_s: float = 0.01,
                     min_gain: float = 0.0, above_fmax="mute", speech_channel: int = 1) -> np.ndarray:
        """The separation silencer (ss_separate_pcm): interleaved int16 (frames, channels), the speech part of the spectrum removed
        inside the (start_s, end_s) regions, the rest as silence_pcm writes it.  Resets the context (ss_reset + ss_add_pcm)."""
        pcm = np.ascontiguousarray(pcm)
        self._need_bytes(pcm, fmt, channels, frames)
        p = separation_params(fade_s, min_gain, above_fmax, speech_channel)
        out = np.empty((frames, channels), dtype=np.int16)
        self._ck(lib().ss_separate_pcm(self._h, _ptr(pcm), fmt, sr, channels, frames, _regions(regions), len(regions), C.byref(p),
                                       _ptr(out)))
        return out

    def separate_pcm_channels(self, pcm: np.ndarray, fmt: int, sr: int, channels: int, frames: int, regions, fade_s: float = 0.01,
                              min_gain: float = 0.0, above_fmax="mute", speech_channel: int = 1) -> np.ndarray:
        """Per-channel separation (ss_separate_pcm_channels): separate_pcm with every channel's gains from its own network passes
        instead of the mono mix's.  Resets the context (ss_reset + ss_add_pcm_channels): files 0 .. channels - 1 are the channels."""
        pcm = np.ascontiguousarray(pcm)
        self._need_bytes(pcm, fmt, channels, frames)
        p = separation_params(fade_s, min_gain, above_fmax, speech_channel)
        out = np.empty((frames, channels), dtype=np.int16)
        self._ck(lib().ss_separate_pcm_channels(self._h, _ptr(pcm), fmt, sr, channels, frames, _regions(regions), len(regions),
                                                C.byref(p), _ptr(out)))
        return out

    def silence_pcm_source(self, pcm: np.ndarray, fmt: int, sr: int, channels: int, frames: int, regions) -> np.ndarray:
        """silence_pcm in the recording's own encoding (ss_silence_pcm_source): uint8 (frames, channels x bytes per sample), the input's
        bytes with the frames of the (start_s, end_s) regions replaced by the encoding's zero."""
        pcm = np.ascontiguousarray(pcm)
        self._need_bytes(pcm, fmt, channels, frames)
        out = np.empty((frames, channels * _BPS[fmt]), dtype=np.uint8)
        self._ck(lib().ss_silence_pcm_source(self._h, _ptr(pcm), fmt, sr, channels, frames, _regions(regions), len(regions), _ptr(out),
                                             out.nbytes))
        return out

    def _separate_source(self, fn, pcm, fmt, sr, channels, frames, regions, fade_s, min_gain, above_fmax, speech_channel):
        pcm = np.ascontiguousarray(pcm)
        self._need_bytes(pcm, fmt, channels, frames)
        p = separation_params(fade_s, min_gain, above_fmax, speech_channel)
        out = np.empty((frames, channels * _BPS[fmt]), dtype=np.uint8)
        self._ck(fn(self._h, _ptr(pcm), fmt, sr, channels, frames, _regions(regions), len(regions), C.byref(p), _ptr(out), out.nbytes))
        return out

    def separate_pcm_source(self, pcm: np.ndarray, fmt: int, sr: int, channels: int, frames: int, regions, fade_s: float = 0.01,
                            min_gain: float = 0.0, above_fmax="mute", speech_channel: int = 1) -> np.ndarray:
        """separate_pcm in the recording's own encoding (ss_separate_pcm_source): uint8 (frames, channels x bytes per sample); the input's
        bytes outside the regions, the separated audio encoded with the decode's own scale (saturated) inside.  Resets the context."""
        return self._separate_source(lib().ss_separate_pcm_source, pcm, fmt, sr, channels, frames, regions, fade_s, min_gain, above_fmax,
                                     speech_channel)

    def separate_pcm_channels_source(self, pcm: np.ndarray, fmt: int, sr: int, channels: int, frames: int, regions, fade_s: float = 0.01,
                                     min_gain: float = 0.0, above_fmax="mute", speech_channel: int = 1) -> np.ndarray:
        """separate_pcm_channels in the recording's own encoding (ss_separate_pcm_channels_source)."""
        return self._separate_source(lib().ss_separate_pcm_channels_source, pcm, fmt, sr, channels, frames, regions, fade_s, min_gain,
                                     above_fmax, speech_channel)

    def box_silence_pcm(self, pcm: np.ndarray, fmt: int, sr: int, channels: int, boxes, *, fade_s: float = 0.01, min_gain: float = 0.0,
                        edge_hz: float = 100.0, encoding: str = "pcm16", frames: int | None = None) -> np.ndarray:
        """The band silencer (ss_box_silence_pcm / _source): inside each box's time range only the box's own frequency band is removed.
        boxes: boxes_array's input.  encoding "pcm16": interleaved int16 (frames, channels), the rest as silence_pcm writes it; "source":
        uint8 (frames, channels x bytes per sample), the input's bytes outside the boxes.  frames: the whole buffer's when not given.
        No model pass; the context's files, results and streams stay as they are."""
        if encoding not in ("pcm16", "source"):
            raise ValueError(f'encoding must be "pcm16" or "source", not {encoding!r}')
        pcm = np.ascontiguousarray(pcm)
        if frames is None:
            if fmt not in _BPS or int(channels) < 1:
                raise ValueError(f"unknown PCM format code {fmt} or channel count {channels}")
            frames = pcm.nbytes // (int(channels) * _BPS[fmt])
        self._need_bytes(pcm, fmt, channels, frames)
        arr = boxes_array(boxes)
        p = BoxParams(float(fade_s), float(min_gain), float(edge_hz))
        bp = _ptr(arr) if len(arr) else None
        if encoding == "source":
            out = np.empty((frames, channels * _BPS[fmt]), dtype=np.uint8)
            self._ck(lib().ss_box_silence_pcm_source(self._h, _ptr(pcm), fmt, sr, channels, frames, bp, len(arr), C.byref(p), _ptr(out), out.nbytes))
        else:
            out = np.empty((frames, channels), dtype=np.int16)
            self._ck(lib().ss_box_silence_pcm(self._h, _ptr(pcm), fmt, sr, channels, frames, bp, len(arr), C.byref(p), _ptr(out)))
        return out

    def separation_maps(self, fid: int, first_bin: int, n_bins: int) -> np.ndarray:
        """Averaged spec-head maps of bins [first_bin, first_bin + n_bins) of file fid: float32 [2, n_bins, 128]."""
        out = np.empty((2, int(n_bins), 128), dtype=np.float32)
        self._ck(lib().ss_separation_maps(self._h, int(fid), int(first_bin), int(n_bins), _ptr(out)))
        return out

    def region_bands(self, fid: int, regions, n_channels: int = 1, q_low: float = .05, q_high: float = .95, speech_channel: int = 1,
                     profile: bool = False):
        """Each region's frequency extent from the spec head's speech map (ss_region_bands): a REGION_BAND_DTYPE array [n] (n_channels
        == 1) or [n, n_channels] (the files fid .. fid + n_channels - 1 of add_pcm_channels); low_hz / high_hz / peak_hz are NaN and the
        band indices -1 where there is no estimate.  profile=True: -> (bands, E) with E float64 [n, (n_channels,) 2, 128]."""
        out, prof = _band_call(lib().ss_region_bands, self._h, (int(fid), int(n_channels)), regions, int(n_channels), q_low, q_high,
                               speech_channel, profile)
        if int(n_channels) == 1:
            out, prof = out[:, 0], (prof[:, 0] if profile else None)
        return (out, prof) if profile else out

    def region_bands_from_maps(self, maps, first_bin: int, regions, q_low: float = .05, q_high: float = .95, speech_channel: int = 1,
                               profile: bool = False):
        """region_bands on maps the caller supplies (ss_region_bands_from_maps): maps float32 [2, n_bins, 128] or [n_signals, 2, n_bins,
        128] for the bins first_bin .., as separation_maps returns them; the result is shaped as region_bands'."""
        maps = np.ascontiguousarray(maps, dtype=np.float32)
        single = maps.ndim == 3
        if single:
            maps = maps[None]
        if maps.ndim != 4 or maps.shape[1] != 2 or maps.shape[3] != 128:
            raise ValueError("maps must be [2, n_bins, 128] or [n_signals, 2, n_bins, 128]")
        ns, nb = maps.shape[0], maps.shape[2]
        out, prof = _band_call(lib().ss_region_bands_from_maps, self._h, (_ptr(maps), ns, int(first_bin), nb), regions, ns, q_low, q_high,
                               speech_channel, profile)
        if single:
            out, prof = out[:, 0], (prof[:, 0] if profile else None)
        return (out, prof) if profile else out

    def debug_set_bands_budget(self, bins: int):
        """Development build only: region_bands covers at most `bins` bins per round of passes (floor 64; <= 0: the product's number)."""
        self._ck(lib().ss_debug_set_bands_budget(self._h, int(bins)))

    def stft512_magnitude(self, samples) -> np.ndarray:
        """|STFT| (n_fft = win = 512, hop 256, centred, zero padded) of a mono float32 signal -> float32 [257, 1 + n // 256]."""
        x = np.ascontiguousarray(samples, dtype=np.float32).reshape(-1)
        nf = int(lib().ss_stft512_frames(x.size))
        out = np.empty((257, nf), dtype=np.float32)
        self._ck(lib().ss_stft512_magnitude(self._h, _ptr(x), x.size, _ptr(out), nf))
        return out

    def add_pcm_device(self, dev_ptr: int, fmt: int, sr: int, channels: int, frames: int) -> int:
        fid = C.c_int(-1)
        self._ck(lib().ss_add_pcm_device(self._h, C.c_void_p(dev_ptr), fmt, sr, channels, frames, C.byref(fid)))
        return fid.value

    def add_pcm_batch_device(self, dev_ptr: int, fmt: int, sr: int, channels: int, frames, host_copy: np.ndarray | None = None) -> int:
        """frames[i] frames per file, files back to back in the device buffer (host_copy: the array that was uploaded there, if
        the caller still has it -- its size is then checked against the frame counts)."""
        fr = np.ascontiguousarray(frames, dtype=np.int64)
        if host_copy is not None:
            self._need_bytes(np.asarray(host_copy), fmt, channels, fr)
        fid = C.c_int(-1)
        self._ck(lib().ss_add_pcm_batch_device(self._h, C.c_void_p(dev_ptr), fmt, sr, channels, _ptr(fr), len(fr), C.byref(fid)))
        return fid.value

    # ---- per-channel ingest: a recording of C channels -> C signals with consecutive file ids, no mixdown ---------------------
    def add_pcm_channels(self, pcm: np.ndarray, fmt: int, sr: int, channels: int, frames: int) -> int:
        """-> first file id; channel c is file first + c, bit for bit what add_pcm stores for that channel's samples as mono PCM."""
        pcm = np.ascontiguousarray(pcm)
        self._need_bytes(pcm, fmt, channels, frames)
        fid = C.c_int(-1)
        self._ck(lib().ss_add_pcm_channels(self._h, _ptr(pcm), fmt, sr, channels, frames, C.byref(fid)))
        return fid.value

    def add_pcm_channels_device(self, dev_ptr: int, fmt: int, sr: int, channels: int, frames: int) -> int:
        fid = C.c_int(-1)
        self._ck(lib().ss_add_pcm_channels_device(self._h, C.c_void_p(dev_ptr), fmt, sr, channels, frames, C.byref(fid)))
        return fid.value

    def add_pcm_channels_batch_device(self, dev_ptr: int, fmt: int, sr: int, channels: int, frames, host_copy: np.ndarray | None = None) -> int:
        """As add_pcm_batch_device: recording r, channel c -> file id first + r * channels + c."""
        fr = np.ascontiguousarray(frames, dtype=np.int64)
        if host_copy is not None:
            self._need_bytes(np.asarray(host_copy), fmt, channels, fr)
        fid = C.c_int(-1)
        self._ck(lib().ss_add_pcm_channels_batch_device(self._h, C.c_void_p(dev_ptr), fmt, sr, channels, _ptr(fr), len(fr), C.byref(fid)))
        return fid.value

    def add_wav_bytes(self, buf) -> tuple[int, WavInfo]:
        info = wav_parse(buf)
        a = np.frombuffer(buf, dtype=np.uint8, count=info.data_bytes, offset=info.data_offset)
        return self.add_pcm(a, info.format, info.sample_rate, info.channels, info.frames), info

    def add_f32_22k(self, x: np.ndarray, padded: bool = False) -> int:
        x = np.ascontiguousarray(x, dtype=np.float32)
        fid = C.c_int(-1)
        fn = lib().ss_add_padded_f32_22k if padded else lib().ss_add_f32_22k
        self._ck(fn(self._h, _ptr(x), x.size, C.byref(fid)))
        return fid.value

    def signal_length(self, fid: int, padded: bool = False) -> int:
        return lib().ss_signal_length(self._h, fid, int(padded))

    def read_signal(self, fid: int, padded: bool = False) -> np.ndarray:
        n = self.signal_length(fid, padded)
        out = np.empty(n, dtype=np.float32)
        self._ck(lib().ss_read_signal(self._h, fid, int(padded), 0, n, _ptr(out)))
        return out

    def device_alloc(self, nbytes: int) -> int:
        p = C.c_void_p()
        self._ck(lib().ss_device_alloc(self._h, nbytes, C.byref(p)))
        return p.value

    def device_free(self, p: int):
        self._ck(lib().ss_device_free(self._h, C.c_void_p(p)))

    def device_upload(self, dst: int, src: np.ndarray):
        src = np.ascontiguousarray(src)
        self._ck(lib().ss_device_upload(self._h, C.c_void_p(dst), _ptr(src), src.nbytes))

    # ---- ingest: the next job's files cross PCIe on the copy stream while the job in flight computes -------------------
    def host_alloc(self, nbytes: int) -> np.ndarray:
        """Page-locked host memory as a uint8 array (free it with host_free; it does not free itself)."""
        p = C.c_void_p()
        self._ck(lib().ss_host_alloc(self._h, int(nbytes), C.byref(p)))
        buf = (C.c_uint8 * int(nbytes)).from_address(p.value)
        a = np.frombuffer(buf, dtype=np.uint8)
        return a

    def host_free(self, a: np.ndarray):
        self._ck(lib().ss_host_free(self._h, C.c_void_p(a.ctypes.data)))

    def upload_wav_batch_async(self, files, dev_dst: int, cap: int):
        """files: uint8 arrays holding RIFF/WAVE images (page-locked ones copy asynchronously).  Header walk of each + one
        asynchronous copy per file of its samples, back to back from dev_dst, on the copy stream -> list of WavInfo.  The arrays
        must stay alive and untouched until upload_wait() / sync(); the next add_pcm*_device waits for the copies on the device."""
        n = len(files)
        ptrs = (C.c_void_p * n)(*[f.ctypes.data for f in files])
        sizes = (C.c_size_t * n)(*[f.nbytes for f in files])
        infos = (WavInfo * n)()
        self._ck(lib().ss_upload_wav_batch_async(self._h, ptrs, sizes, n, C.c_void_p(dev_dst), int(cap), infos))
        self._upload_keep = (files, ptrs, sizes)
        return infos

    def device_upload_async(self, dst: int, src: np.ndarray):
        src = np.ascontiguousarray(src)
        self._upload_keep = src
        self._ck(lib().ss_device_upload_async(self._h, C.c_void_p(dst), _ptr(src), src.nbytes))

    def upload_wait(self):
        self._ck(lib().ss_upload_wait(self._h))
        self._upload_keep = None

    def features(self, fid: int, starts, discard: bool = False):
        s = np.ascontiguousarray(starts, dtype=np.int64)
        out = None if discard else np.empty((len(s), 128, 256), dtype=np.float32)
        self._ck(lib().ss_features(self._h, fid, _ptr(s), len(s), _ptr(out)))
        return out

    def infer_windows(self, fid: int, starts, want_spec: bool = False):
        s = np.ascontiguousarray(starts, dtype=np.int64)
        mask = np.empty((len(s), 1, 256), dtype=np.float32)
        spec = np.empty((len(s), 2, 128, 256), dtype=np.float32) if want_spec else None
        self._ck(lib().ss_infer_windows(self._h, fid, _ptr(s), len(s), _ptr(mask), _ptr(spec)))
        return spec, mask

    def run(self, threshold: float = 0.1, break_s: float = 0.5, progress=None, stop_flag=None):
        """progress(done, total) is called between chunks; stop_flag: ctypes.c_int polled between chunks."""
        cb = None
        if progress is not None:
            cb = PROGRESS_FN(lambda _u, d, t: progress(d, t))
        self._cb_keep = cb
        rc = lib().ss_run(self._h, threshold, break_s, C.cast(cb, C.c_void_p) if cb else None, None,
                          C.cast(C.byref(stop_flag), C.c_void_p) if stop_flag is not None else None)
        self._cb_keep = None
        if rc == SS_ERR_STOPPED:
            return False
        self._ck(rc)
        return True

    def run_begin(self, threshold: float = 0.1, break_s: float = 0.5, track: bool = False):
        """First half of run(): plan and enqueue; returns while the device works.  The context takes no other work until run_end().
        track: an event behind every pass, for run_poll()."""
        fn = lib().ss_run_begin_tracked if track else lib().ss_run_begin
        self._ck(fn(self._h, threshold, break_s))

    def run_poll(self, progress=None, block: bool = True):
        """Progress of the run started with run_begin(track=True): progress(done, total) for every value of the reference's sequence
        (32, 64, ..., total windows) that has completed since the last call; block: wait for all of them."""
        cb = PROGRESS_FN(lambda _u, d, t: progress(d, t)) if progress is not None else None
        self._ck(lib().ss_run_poll(self._h, C.cast(cb, C.c_void_p) if cb else None, None, int(bool(block))))

    def run_end(self):
        """Second half of run(): wait for the device, find the regions."""
        self._ck(lib().ss_run_end(self._h))

    def run_from_logits(self, logits: np.ndarray, threshold: float = 0.1, break_s: float = 0.5):
        """The tail of run() on per-window logits computed elsewhere (window ranges of one recording on several GPUs):
        logits [total windows of the files added since reset()][256]."""
        lg = np.ascontiguousarray(logits, dtype=np.float32).reshape(-1, 256)
        self._ck(lib().ss_run_from_logits(self._h, _ptr(lg), lg.shape[0], threshold, break_s))

    def debug_fail_workspace_alloc(self, nth: int):
        """Development build only (SOFTSPOKEN_LIB=libsoftspoken_hip_dev.so)."""
        self._ck(lib().ss_debug_fail_workspace_alloc(self._h, int(nth)))

    def debug_set_separation_budget(self, frames: int):
        """Development build only: separate_pcm holds at most `frames` STFT frames at once (floor 16; <= 0: the product's number)."""
        self._ck(lib().ss_debug_set_separation_budget(self._h, int(frames)))

    def debug_activation(self, name: str, first: int, n: int) -> dict:
        """Development build only: tensor `name` ("h1" ... "s9", "feat", "flat_part") of the last network pass, windows [first, first + n)
        of that pass.  -> dict(planes=[raw stored planes, [n][H][W][C]: fp32 / bf16 as uint16 / f16 high, f16 low],
        value=float64 [n][H][W][C] in normalised units (the stored planes decoded; f16x2: high + low), exponents=int32 [C]: the
        value of channel c is 2^-exponents[c] x the normalised one)."""
        L = lib()
        shape = np.zeros(4, dtype=np.int32)
        key = name.encode()
        self._ck(L.ss_debug_activation(self._h, key, 0, 0, 0, None, 0, _ptr(shape), None))
        H, W, Ch, es = (int(v) for v in shape)
        exps = np.zeros(Ch, dtype=np.int32)
        self._ck(L.ss_debug_activation(self._h, key, 0, 0, 0, None, 0, None, _ptr(exps)))
        dt = {4: np.float32, 2: np.uint16}[es]
        two = name not in ("feat", "flat_part") and self.precision == "f16x2"
        planes = []
        for plane in range(2 if two else 1):
            a = np.empty((n, H, W, Ch), dtype=dt)
            if n:                                         # (n == 0: the model's shape and exponents, no pass needed)
                self._ck(L.ss_debug_activation(self._h, key, plane, first, n, _ptr(a), a.nbytes, None, None))
            planes.append(a)
        if two:
            value = planes[0].view(np.float16).astype(np.float64) + planes[1].view(np.float16).astype(np.float64)
        elif es == 2:
            value = (planes[0].astype(np.uint32) << 16).view(np.float32).astype(np.float64)
        else:
            value = planes[0].astype(np.float64)
        return dict(planes=planes, value=value, exponents=exps)

    def workspace_bytes(self) -> int:
        return int(lib().ss_workspace_bytes(self._h))

    def num_windows(self, fid: int) -> int:
        return lib().ss_num_windows(self._h, fid)

    def window_logits(self, fid: int) -> np.ndarray:
        w = self.num_windows(fid)
        out = np.empty((w, 1, 256), dtype=np.float32)
        self._ck(lib().ss_get_window_logits(self._h, fid, _ptr(out), w))
        return out

    def avg(self, fid: int):
        n = C.c_int64(0)
        self._ck(lib().ss_get_avg(self._h, fid, None, None, 0, C.byref(n)))
        a = np.empty(n.value, dtype=np.float64)
        idx = np.empty(n.value, dtype=np.int64)
        self._ck(lib().ss_get_avg(self._h, fid, _ptr(a), _ptr(idx), n.value, C.byref(n)))
        return a, idx

    def regions(self, fid: int):
        n = C.c_int64(0)
        self._ck(lib().ss_get_regions(self._h, fid, None, 0, C.byref(n)))
        arr = (Region * max(1, n.value))()
        self._ck(lib().ss_get_regions(self._h, fid, arr, n.value, C.byref(n)))
        return [(arr[i].start, arr[i].end) for i in range(n.value)]

    def regions_batch(self, first: int, n_files: int):
        """-> (counts int64[n_files], regions float64[total, 2]) for files first .. first + n_files - 1, one foreign call each way."""
        n = C.c_int64(0)
        self._ck(lib().ss_get_regions_batch(self._h, first, n_files, None, None, 0, C.byref(n)))
        counts = np.zeros(max(n_files, 1), dtype=np.int64)
        out = np.zeros((max(n.value, 1), 2), dtype=np.float64)
        self._ck(lib().ss_get_regions_batch(self._h, first, n_files, _ptr(counts), _ptr(out), n.value, C.byref(n)))
        return counts[:n_files], out[:n.value]

    def regions_union(self, first: int, n_channels: int):
        """The merged table ("speech on any channel") of files first .. first + n_channels - 1 of the ended run."""
        n = C.c_int64(0)
        self._ck(lib().ss_get_regions_union(self._h, int(first), int(n_channels), None, 0, C.byref(n)))
        arr = (Region * max(1, n.value))()
        self._ck(lib().ss_get_regions_union(self._h, int(first), int(n_channels), arr, n.value, C.byref(n)))
        return [(arr[i].start, arr[i].end) for i in range(n.value)]

    def region_peaks(self, first: int, n_channels: int) -> np.ndarray:
        """float64 [merged regions, n_channels]: each channel's highest averaged score inside each region of regions_union()."""
        n = C.c_int64(0)
        self._ck(lib().ss_get_region_peaks(self._h, int(first), int(n_channels), None, 0, C.byref(n)))
        out = np.empty((n.value, int(n_channels)), dtype=np.float64)
        if n.value:
            self._ck(lib().ss_get_region_peaks(self._h, int(first), int(n_channels), _ptr(out), n.value, C.byref(n)))
        return out

    def sync(self):
        self._ck(lib().ss_sync(self._h))

    def reset_stats(self):
        self._ck(lib().ss_reset_kernel_stats(self._h))

    def kernel_stats(self):
        n = C.c_int(0)
        self._ck(lib().ss_get_kernel_stats(self._h, None, 0, C.byref(n)))
        arr = (KernelStat * max(1, n.value))()
        self._ck(lib().ss_get_kernel_stats(self._h, arr, n.value, C.byref(n)))
        return [dict(name=arr[i].name.decode(), launches=arr[i].launches, total_ms=arr[i].total_ms, flops=arr[i].flops,
                     bytes=arr[i].bytes, issued_flops=arr[i].issued_flops) for i in range(n.value)]

    def last_run_device_ms(self) -> float:
        return lib().ss_last_run_device_ms(self._h)

    # ---- streaming detection (ss_stream_*): one recording's PCM in pieces; see include/softspoken.h ----------------------------
    def stream_open(self, fmt: int, sr: int, channels: int, threshold: float = 0.1, break_s: float = 0.5) -> int:
        sid = C.c_int(-1)
        self._ck(lib().ss_stream_open(self._h, int(fmt), int(sr), int(channels), float(threshold), float(break_s), C.byref(sid)))
        return sid.value

    def stream_open_output(self, fmt: int, sr: int, channels: int, threshold: float = 0.1, break_s: float = 0.5, erase=None) -> int:
        """A stream that also returns its frames as final 16-bit PCM with the detected speech zeroed (stream_output after every
        step).  erase: None, dict(pad_s=, min_len_s=) or a pair."""
        sid = C.c_int(0)
        e = _erase(erase)
        self._ck(lib().ss_stream_open_output(self._h, int(fmt), int(sr), int(channels), float(threshold), float(break_s), C.byref(e), C.byref(sid)))
        return sid.value

    def stream_open_channels(self, fmt: int, sr: int, channels: int, threshold: float = 0.1, break_s: float = 0.5, erase=None,
                             with_output: bool = False) -> int:
        """A stream whose channels are detected each alone (one lane per channel, one merged table: stream_regions / stream_avg give
        "speech on any channel", stream_avg_channel a channel's own series, stream_region_peaks the channels' peaks per region).
        erase None and with_output False: detection only; otherwise a stream with output, erase as stream_open_output's."""
        sid = C.c_int(-1)
        e = _erase(erase)
        self._ck(lib().ss_stream_open_channels(self._h, int(fmt), int(sr), int(channels), float(threshold), float(break_s),
                                               C.byref(e) if erase is not None else None, int(bool(with_output)), C.byref(sid)))
        return sid.value

    def stream_open_bands(self, fmt: int, sr: int, channels: int, threshold: float = 0.1, break_s: float = 0.5, erase=None,
                          with_output: bool = False, each_channel: bool = False, q_low: float = .05, q_high: float = .95,
                          speech_channel: int = 1, profile: bool = False) -> int:
        """A stream that returns with every region its frequency extent (stream_bands after every step; ss_stream_open_bands): any
        combination of output (erase / with_output as stream_open_channels) and each_channel.  Needs the default window step."""
        sid = C.c_int(-1)
        e = _erase(erase)
        p = band_params(q_low, q_high, speech_channel)
        self._ck(lib().ss_stream_open_bands(self._h, int(fmt), int(sr), int(channels), float(threshold), float(break_s),
                                            C.byref(e) if erase is not None else None, int(bool(with_output)), int(bool(each_channel)),
                                            C.byref(p), int(bool(profile)), C.byref(sid)))
        return sid.value

    def stream_bands(self, sid: int, lanes: int = 1, profile: bool = False):
        """(REGION_BAND_DTYPE records [regions the last step returned, lanes], profiles float64 [regions, lanes, 2, 128] or None)."""
        n = C.c_int64(0)
        self._ck(lib().ss_stream_bands(self._h, int(sid), None, None, 0, C.byref(n)))
        out = np.zeros((n.value, int(lanes)), dtype=REGION_BAND_DTYPE)
        prof = np.zeros((n.value, int(lanes), 2, 128), dtype=np.float64) if profile else None
        if n.value or profile:                                # (a profile asked of a stream opened without one is refused, regions or not)
            pp = (prof if n.value else np.zeros(1)) if profile else None
            self._ck(lib().ss_stream_bands(self._h, int(sid), _ptr(out) if n.value else None, _ptr(pp) if profile else None, n.value, C.byref(n)))
        return out, prof

    def stream_avg_channel(self, sid: int, channel: int):
        """stream_avg of one channel's lane of an each-channel stream (channel 0 of a mix stream: stream_avg)."""
        n = C.c_int64(0)
        self._ck(lib().ss_stream_avg_channel(self._h, int(sid), int(channel), None, None, 0, C.byref(n)))
        a = np.empty(n.value, dtype=np.float64)
        idx = np.empty(n.value, dtype=np.int64)
        if n.value:
            self._ck(lib().ss_stream_avg_channel(self._h, int(sid), int(channel), _ptr(a), _ptr(idx), n.value, C.byref(n)))
        return a, idx

    def stream_region_peaks(self, sid: int, channels: int) -> np.ndarray:
        """float64 [regions the last step returned, channels]: each channel's highest averaged score inside each of them."""
        n = C.c_int64(0)
        self._ck(lib().ss_stream_region_peaks(self._h, int(sid), None, 0, C.byref(n)))
        out = np.empty((n.value, int(channels)), dtype=np.float64)
        if n.value:
            self._ck(lib().ss_stream_region_peaks(self._h, int(sid), _ptr(out), n.value, C.byref(n)))
        return out

    def stream_output(self, sid: int, channels: int):
        """The frames the last step returned -> (first_frame, int16 array [n, channels])."""
        first, n = C.c_int64(0), C.c_int64(0)
        self._ck(lib().ss_stream_output(self._h, int(sid), None, 0, C.byref(first), C.byref(n)))
        out = np.zeros((n.value, int(channels)), dtype=np.int16)
        if n.value:
            self._ck(lib().ss_stream_output(self._h, int(sid), _ptr(out), n.value, C.byref(first), C.byref(n)))
        return first.value, out

    def stream_open_source(self, fmt: int, sr: int, channels: int, threshold: float = 0.1, break_s: float = 0.5, erase=None,
                           each_channel: bool = False) -> int:
        """A stream with output in its own encoding (ss_stream_open_source): stream_output_bytes after every step.  each_channel as
        stream_open_channels; erase None: pad_s = min_len_s = 0."""
        sid = C.c_int(-1)
        e = _erase(erase)
        self._ck(lib().ss_stream_open_source(self._h, int(fmt), int(sr), int(channels), float(threshold), float(break_s), C.byref(e),
                                             int(bool(each_channel)), C.byref(sid)))
        return sid.value

    def stream_output_bytes(self, sid: int, frame_bytes: int):
        """The frames the last step of a source-output stream returned -> (first_frame, uint8 array [n, frame_bytes]), frame_bytes =
        channels x bytes per sample of the stream's encoding."""
        first, n = C.c_int64(0), C.c_int64(0)
        self._ck(lib().ss_stream_output_bytes(self._h, int(sid), None, 0, C.byref(first), C.byref(n)))
        out = np.zeros((n.value, int(frame_bytes)), dtype=np.uint8)
        if n.value:
            self._ck(lib().ss_stream_output_bytes(self._h, int(sid), _ptr(out), out.nbytes, C.byref(first), C.byref(n)))
        return first.value, out

    def stream_output_info(self, sid: int) -> dict:
        info = StreamOutputInfo()
        self._ck(lib().ss_stream_get_output_info(self._h, int(sid), C.byref(info)))
        return {k: getattr(info, k) for k, _ in StreamOutputInfo._fields_}

    def stream_push(self, sid: int, pcm: np.ndarray, frames: int | None = None, channels: int = 1, fmt: int | None = None):
        """pcm: interleaved samples of the stream's encoding (any dtype whose bytes are that encoding); frames defaults to
        pcm.nbytes // (channels x bytes per sample) when fmt is given, else to len(pcm) // channels."""
        a = np.ascontiguousarray(pcm)
        if frames is None:
            frames = a.nbytes // (int(channels) * _BPS[fmt]) if fmt is not None else (a.shape[0] if a.ndim > 1 else a.size // int(channels))
        if fmt is not None:
            self._need_bytes(a, fmt, channels, frames)
        self._ck(lib().ss_stream_push(self._h, int(sid), _ptr(a) if a.size else None, int(frames)))

    def stream_close(self, sid: int):
        self._ck(lib().ss_stream_close(self._h, int(sid)))

    def stream_step(self):
        self._ck(lib().ss_stream_step(self._h))

    def stream_regions(self, sid: int):
        n = C.c_int64(0)
        self._ck(lib().ss_stream_regions(self._h, int(sid), None, 0, C.byref(n)))
        arr = (Region * max(1, n.value))()
        self._ck(lib().ss_stream_regions(self._h, int(sid), arr, n.value, C.byref(n)))
        return [(arr[i].start, arr[i].end) for i in range(n.value)]

    def stream_avg(self, sid: int):
        n = C.c_int64(0)
        self._ck(lib().ss_stream_avg(self._h, int(sid), None, None, 0, C.byref(n)))
        a = np.empty(n.value, dtype=np.float64)
        idx = np.empty(n.value, dtype=np.int64)
        if n.value:
            self._ck(lib().ss_stream_avg(self._h, int(sid), _ptr(a), _ptr(idx), n.value, C.byref(n)))
        return a, idx

    def stream_info(self, sid: int) -> dict:
        info = StreamInfo()
        self._ck(lib().ss_stream_get_info(self._h, int(sid), C.byref(info)))
        return {k: getattr(info, k) for k, _ in StreamInfo._fields_}

    def stream_free(self, sid: int):
        self._ck(lib().ss_stream_free(self._h, int(sid)))

    def stream_export(self, sid: int) -> bytes:
        n = C.c_int64(0)
        self._ck(lib().ss_stream_export(self._h, int(sid), None, 0, C.byref(n)))
        buf = np.empty(n.value, dtype=np.uint8)
        self._ck(lib().ss_stream_export(self._h, int(sid), _ptr(buf), n.value, C.byref(n)))
        return buf.tobytes()

    def stream_import(self, image: bytes) -> int:
        a = np.frombuffer(image, dtype=np.uint8)
        sid = C.c_int(-1)
        self._ck(lib().ss_stream_import(self._h, _ptr(a), a.size, C.byref(sid)))
        return sid.value
