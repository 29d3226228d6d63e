"""ctypes binding to ``libvfilter_hip.so`` (the C ABI declared in ``include/vfilter.h``).

The reference's filter call is ``cv2.bitwise_not(frame)`` (inverter.py:41), a Python call
into OpenCV's C++ core.  Here the same call goes through ctypes into hand-written gfx950
HIP kernels.  ctypes releases the GIL for the duration of each foreign call, so a worker's
transport threads keep running while a batch is on the GPU.

There is no fallback: if the library is missing or no gfx950 device is present, the calls
raise.  (The CPU oracle under ``oracle/`` is test infrastructure and is never imported here.)
"""
from __future__ import annotations

import atexit
import ctypes
import os
import threading
from typing import Optional, Sequence

import numpy as np

LIB_NAME = "libvfilter_hip.so"
ABI_VERSION = 3

VF_OK = 0
VF_E_INVALID = -1
VF_E_HIP = -2
VF_E_NOMEM = -3
VF_E_NODEVICE = -4
VF_E_JPEG = -5

_c_int_p = ctypes.POINTER(ctypes.c_int)
_c_float_p = ctypes.POINTER(ctypes.c_float)
_vp = ctypes.c_void_p
_sz = ctypes.c_size_t
_u8p = ctypes.c_void_p  # passed as raw addresses

# name -> (restype, argtypes); must list every entry point of include/vfilter.h
SIGNATURES = {
    "vf_get_abi_version": (ctypes.c_int, []),
    "vf_status_string": (ctypes.c_char_p, [ctypes.c_int]),
    "vf_device_count": (ctypes.c_int, [_c_int_p]),
    "vf_device_pci_bus_id": (ctypes.c_int, [ctypes.c_int, ctypes.c_char_p, ctypes.c_int]),
    "vf_create": (ctypes.c_int, [ctypes.c_int, _sz, ctypes.c_int, ctypes.POINTER(_vp)]),
    "vf_destroy": (ctypes.c_int, [_vp]),
    "vf_last_error": (ctypes.c_char_p, [_vp]),
    "vf_last_hip_error": (ctypes.c_int, [_vp]),
    "vf_ctx_device": (ctypes.c_int, [_vp, _c_int_p]),
    "vf_invert_host": (ctypes.c_int, [_vp, _u8p, _u8p, _sz]),
    "vf_invert_batch_host": (ctypes.c_int, [_vp, _u8p, _u8p, _sz, ctypes.c_int]),
    "vf_invert_frames_host": (ctypes.c_int, [_vp, _vp, _vp, _vp, ctypes.c_int]),
    "vf_invert_frames_async": (ctypes.c_int, [_vp, _vp, _vp, _vp, ctypes.c_int, ctypes.POINTER(ctypes.c_uint64)]),
    "vf_wait": (ctypes.c_int, [_vp, ctypes.c_uint64, _c_float_p]),
    "vf_query": (ctypes.c_int, [_vp, ctypes.c_uint64, _c_int_p]),
    "vf_invert_device": (ctypes.c_int, [_vp, _vp, _vp, _sz, _vp]),
    "vf_invert_device_frames": (ctypes.c_int, [_vp, _vp, _vp, _vp, ctypes.c_int, _sz, _vp]),
    "vf_alloc_device": (ctypes.c_int, [_vp, _sz, ctypes.POINTER(_vp)]),
    "vf_free_device": (ctypes.c_int, [_vp, _vp]),
    "vf_alloc_host": (ctypes.c_int, [_vp, _sz, ctypes.POINTER(_vp)]),
    "vf_free_host": (ctypes.c_int, [_vp, _vp]),
    "vf_host_register": (ctypes.c_int, [_vp, _vp, _sz]),
    "vf_host_unregister": (ctypes.c_int, [_vp, _vp]),
    "vf_upload": (ctypes.c_int, [_vp, _vp, _vp, _sz, _vp]),
    "vf_download": (ctypes.c_int, [_vp, _vp, _vp, _sz, _vp]),
    "vf_memset_device": (ctypes.c_int, [_vp, _vp, ctypes.c_int, _sz, _vp]),
    "vf_sync": (ctypes.c_int, [_vp, _vp]),
    "vf_elapsed_ms": (ctypes.c_int, [_vp, _c_float_p]),
    "vf_last_timeline": (ctypes.c_int, [_vp, _c_float_p, ctypes.POINTER(_sz), ctypes.c_int, _c_int_p]),
    "vf_bench_device_ring": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_int, _sz, ctypes.c_int, _vp, _c_float_p,
                                            _c_float_p]),
    "vf_jpeg_header": (ctypes.c_int, [_vp, _sz, _c_int_p, _c_int_p, _c_int_p, _c_int_p]),
    "vf_jpeg_set_max_pixels": (ctypes.c_int, [_vp, ctypes.c_uint64]),
    "vf_jpeg_buffer_size": (_sz, [ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    "vf_jpeg_encode": (ctypes.c_int, [_vp, _vp, _vp, _vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                      ctypes.c_int, _vp, _vp, _vp]),
    "vf_jpeg_decode": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, _vp, _vp]),
    "vf_jpeg_invert": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, _vp,
                                      _vp, _vp]),
    "vf_jpeg_invert_submit": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                             ctypes.POINTER(ctypes.c_uint64)]),
    "vf_jpeg_invert_query": (ctypes.c_int, [_vp, ctypes.c_uint64, _c_int_p]),
    "vf_jpeg_invert_wait": (ctypes.c_int, [_vp, ctypes.c_uint64, ctypes.POINTER(_sz)]),
    "vf_jpeg_invert_fetch": (ctypes.c_int, [_vp, ctypes.c_uint64, _vp, _sz, _vp, _vp]),
    "vf_jpeg_invert_scatter": (ctypes.c_int, [_vp, ctypes.c_uint64, _vp, _vp, _vp, ctypes.POINTER(ctypes.c_int)]),
    "vf_jpeg_bench_invert": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                            ctypes.c_int, _c_float_p, _c_float_p]),
    "vf_lut_device": (ctypes.c_int, [_vp, _vp, _vp, _sz, _u8p, ctypes.c_int, _vp]),
    "vf_lut_frames_host": (ctypes.c_int, [_vp, _vp, _vp, _vp, ctypes.c_int, _u8p, ctypes.c_int]),
    "vf_jpeg_lut": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_int, _u8p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                   ctypes.c_int, _vp, _vp, _vp]),
    "vf_jpeg_lut_submit": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_int, _u8p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                          ctypes.c_int, ctypes.POINTER(ctypes.c_uint64)]),
    "vf_jpeg_bench_lut": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_int, _u8p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                         ctypes.c_int, ctypes.c_int, _c_float_p, _c_float_p]),
    "vf_conv_device": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, _vp, ctypes.c_int,
                                      ctypes.c_int, ctypes.c_int, ctypes.c_int, _vp]),
    "vf_conv_frames_host": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, ctypes.c_int, ctypes.c_int, _vp, ctypes.c_int,
                                           ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    "vf_jpeg_conv": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_int, _vp, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                    ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, _vp, _vp, _vp]),
    "vf_jpeg_conv_submit": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_int, _vp, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                           ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                           ctypes.POINTER(ctypes.c_uint64)]),
    "vf_jpeg_bench_conv": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_int, _vp, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                          ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                          _c_float_p, _c_float_p]),
    "vf_rank_device": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, _vp,
                                      ctypes.c_int, ctypes.c_int, ctypes.c_int, _vp]),
    "vf_rank_frames_host": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, _vp,
                                           ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    "vf_jpeg_rank": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_int, ctypes.c_int, _vp, ctypes.c_int, ctypes.c_int,
                                    ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, _vp, _vp, _vp]),
    "vf_jpeg_rank_submit": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_int, ctypes.c_int, _vp, ctypes.c_int, ctypes.c_int,
                                           ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                           ctypes.POINTER(ctypes.c_uint64)]),
    "vf_jpeg_bench_rank": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_int, ctypes.c_int, _vp, ctypes.c_int, ctypes.c_int,
                                          ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                          _c_float_p, _c_float_p]),
    "vf_mix_tile_bytes": (_sz, []),
    "vf_mix_device": (ctypes.c_int, [_vp, _vp, _vp, _sz, _vp, ctypes.c_int, ctypes.c_int, _vp]),
    "vf_mix_frames_host": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, ctypes.c_int, ctypes.c_int, _vp, ctypes.c_int,
                                          ctypes.c_int]),
    "vf_jpeg_mix": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_int, _vp, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                   ctypes.c_int, ctypes.c_int, _vp, _vp, _vp]),
    "vf_jpeg_mix_submit": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_int, _vp, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                          ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_uint64)]),
    "vf_jpeg_bench_mix": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_int, _vp, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                         ctypes.c_int, ctypes.c_int, ctypes.c_int, _c_float_p, _c_float_p]),
    "vf_sep_tile": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, _c_int_p, _c_int_p]),
    "vf_sep_device": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, _vp, ctypes.c_int, _vp,
                                     ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, _vp]),
    "vf_sep_frames_host": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, ctypes.c_int, ctypes.c_int, _vp, ctypes.c_int, _vp,
                                          ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    "vf_jpeg_sep": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_int, _vp, ctypes.c_int, _vp, ctypes.c_int, ctypes.c_int,
                                   ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                   _vp, _vp, _vp]),
    "vf_jpeg_sep_submit": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_int, _vp, ctypes.c_int, _vp, ctypes.c_int,
                                          ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                          ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_uint64)]),
    "vf_jpeg_bench_sep": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_int, _vp, ctypes.c_int, _vp, ctypes.c_int, ctypes.c_int,
                                         ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                         ctypes.c_int, ctypes.c_int, _c_float_p, _c_float_p]),
    "vf_hist_device": (ctypes.c_int, [_vp, _vp, _sz, ctypes.c_int, _vp, _vp]),
    "vf_hist_frames_host": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_int, ctypes.c_int, _vp]),
    "vf_level_device": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                       ctypes.c_int, ctypes.c_int, ctypes.c_int, _vp]),
    "vf_level_frames_host": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                            ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    "vf_jpeg_level": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                     ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, _vp, _vp, _vp]),
    "vf_jpeg_level_submit": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                            ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                            ctypes.POINTER(ctypes.c_uint64)]),
    "vf_jpeg_bench_level": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                           ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                           ctypes.c_int, _c_float_p, _c_float_p]),
    "vf_clahe_device": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                       ctypes.c_int, ctypes.c_int, _vp]),
    "vf_clahe_frames_host": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                            ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    "vf_jpeg_clahe": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                     ctypes.c_int, ctypes.c_int, ctypes.c_int, _vp, _vp, _vp]),
    "vf_jpeg_clahe_submit": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                            ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                            ctypes.POINTER(ctypes.c_uint64)]),
    "vf_jpeg_bench_clahe": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                           ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                           _c_float_p, _c_float_p]),
    "vf_warp_device": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, _vp, ctypes.c_int,
                                      ctypes.c_int, ctypes.c_int, _vp, _vp]),
    "vf_warp_frames_host": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, ctypes.c_int, ctypes.c_int, _vp, ctypes.c_int,
                                           ctypes.c_int, ctypes.c_int, _vp]),
    "vf_jpeg_warp": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_int, _vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, _vp,
                                    ctypes.c_int, ctypes.c_int, ctypes.c_int, _vp, _vp, _vp]),
    "vf_jpeg_warp_submit": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_int, _vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, _vp,
                                           ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_uint64)]),
    "vf_jpeg_bench_warp": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_int, _vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, _vp,
                                          ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, _c_float_p, _c_float_p]),
    "vf_resize_out_size": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_double,
                                          ctypes.c_double, ctypes.c_int, _vp, _vp]),
    "vf_resize_device": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                        ctypes.c_double, ctypes.c_double, ctypes.c_int, _vp]),
    "vf_resize_frames_host": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                             ctypes.c_double, ctypes.c_double, ctypes.c_int]),
    "vf_jpeg_resize": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_double,
                                      ctypes.c_double, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, _vp, _vp, _vp]),
    "vf_jpeg_resize_submit": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_double,
                                             ctypes.c_double, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                             ctypes.POINTER(ctypes.c_uint64)]),
    "vf_jpeg_bench_resize": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_double,
                                            ctypes.c_double, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                            ctypes.c_int, _c_float_p, _c_float_p]),
    "vf_chain_out_size": (ctypes.c_int, [_vp, _vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, _vp, _vp]),
    "vf_binary_device": (ctypes.c_int, [_vp, _vp, _vp, _vp, _sz, ctypes.c_int, _vp]),
    "vf_chain_frames_host": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, ctypes.c_int, ctypes.c_int, _vp, ctypes.c_int]),
    "vf_jpeg_chain": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_int, _vp, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                     ctypes.c_int, _vp, _vp, _vp]),
    "vf_jpeg_chain_submit": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_int, _vp, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                            ctypes.c_int, ctypes.POINTER(ctypes.c_uint64)]),
    "vf_jpeg_bench_chain": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_int, _vp, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                           ctypes.c_int, ctypes.c_int, _c_float_p, _c_float_p]),
}

STEP_TABLE, STEP_CONV, STEP_RANK, STEP_BINARY = 0, 1, 2, 3  # VF_STEP_* (include/vfilter.h)
STEP_MIX = 5                                                # VF_STEP_MIX: 4 names no kind and stays refused
STEP_SEP = 7                                                # VF_STEP_SEP: 6 stays refused as well
STEP_LEVEL = 8                                              # VF_STEP_LEVEL: 9 stays refused as well
LEVEL_EQUALIZE, LEVEL_STRETCH = 0, 1                        # VF_LEVEL_*
STEP_CLAHE = 10                                             # VF_STEP_CLAHE: 11 stays refused as well
STEP_WARP = 12                                              # VF_STEP_WARP: 13 stays refused as well
STEP_RESIZE = 14                                            # VF_STEP_RESIZE: 15 stays refused as well
INTER_NEAREST, INTER_LINEAR, INTER_AREA = 0, 1, 3           # VF_INTER_*: cv2's values
CHAIN_MAX_STEPS = 8                                         # VF_CHAIN_MAX_STEPS
ROUND_HALF_EVEN, ROUND_HALF_UP = 0, 1                       # VF_ROUND_*


class Step(ctypes.Structure):
    """``vf_step`` of include/vfilter.h: one step of a filter chain's program."""
    _fields_ = [("kind", ctypes.c_int), ("a", ctypes.c_int), ("b", ctypes.c_int), ("op", ctypes.c_int),
                ("data", ctypes.c_void_p), ("kw", ctypes.c_int), ("kh", ctypes.c_int), ("shift", ctypes.c_int),
                ("border", ctypes.c_int), ("channels", ctypes.c_int)]


class VFilterError(RuntimeError):
    """A libvfilter_hip call failed.  ``status`` is the VF_E_* code, ``hip_error`` the hipError_t."""

    def __init__(self, message: str, status: int = VF_E_HIP, hip_error: int = 0):
        super().__init__(message)
        self.status = status
        self.hip_error = hip_error


_lib: Optional[ctypes.CDLL] = None
_lib_lock = threading.Lock()


def library_path() -> str:
    """Path of the in-tree library (override with ``VFILTER_LIB``)."""
    return os.environ.get("VFILTER_LIB") or os.path.join(os.path.dirname(os.path.abspath(__file__)), LIB_NAME)


def load_library() -> ctypes.CDLL:
    """Load libvfilter_hip.so once and declare its signatures.  Raises if it is absent."""
    global _lib
    with _lib_lock:
        if _lib is not None:
            return _lib
        path = library_path()
        if not os.path.exists(path):
            raise VFilterError(
                f"{LIB_NAME} not found at {path}; build it with `make` (hipcc --offload-arch=gfx950)",
                VF_E_NODEVICE)
        lib = ctypes.CDLL(path)
        for name, (restype, argtypes) in SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype = restype
            fn.argtypes = argtypes
        got = lib.vf_get_abi_version()
        if got != ABI_VERSION:
            raise VFilterError(f"{path}: ABI version {got}, binding expects {ABI_VERSION}", VF_E_INVALID)
        _lib = lib
        return lib


def device_count() -> int:
    lib = load_library()
    n = ctypes.c_int(0)
    lib.vf_device_count(ctypes.byref(n))
    return n.value


def device_pci_bus_id(device: int) -> str:
    """PCI address ("dddd:bb:dd.f") of HIP device ``device``."""
    lib = load_library()
    buf = ctypes.create_string_buffer(64)
    st = lib.vf_device_pci_bus_id(int(device), buf, 64)
    if st != VF_OK:
        raise VFilterError(lib.vf_last_error(None).decode(), st, lib.vf_last_hip_error(None))
    return buf.value.decode()


def _addr(a) -> int:
    """Address of a numpy array / writable buffer / int pointer."""
    if isinstance(a, int):
        return a
    if isinstance(a, np.ndarray):
        return a.ctypes.data
    if isinstance(a, (bytes, bytearray, memoryview)):
        return np.frombuffer(a, dtype=np.uint8).ctypes.data
    raise TypeError(f"cannot take the address of {type(a).__name__}")


class _PinnedBlock:
    """A block of a context's pinned arena seen as an array (``np.asarray(block)``): the array
    keeps the block alive, and the block goes back to the arena when the last view of it dies."""

    def __init__(self, arena: "_PinnedArena", ptr: int, cap: int, shape, dtype):
        self._arena, self.ptr, self.cap = arena, ptr, cap
        self.__array_interface__ = {"shape": tuple(shape), "typestr": np.dtype(dtype).str,
                                    "data": (ptr, False), "version": 3}

    def __del__(self):
        try:
            self._arena.release(self.ptr, self.cap)
        except Exception:
            pass


class _PinnedArena:
    """Page-locked, device-mapped result buffers of one context (vf_alloc_host: on the GPU's NUMA
    node, noted as mapped), recycled by size.  An array from here is a destination the invert
    kernel writes directly over PCIe (no staging, no copy-out) -- the drop-in's result of
    ``bitwise_not(frame)`` (inverter.py:41) and the worker's receive buffers.  Free blocks beyond
    ``keep_bytes`` are returned to the library; blocks still referenced by arrays keep the context
    alive past ``close`` (its memory must outlive them)."""

    def __init__(self, ctx: "Context", keep_bytes: int = 256 << 20, cap_bytes: Optional[int] = None):
        self._ctx = ctx
        self._lock = threading.Lock()
        self._free: dict = {}
        self._free_bytes = 0
        self._keep = keep_bytes
        # page-locked bytes held by live result arrays; ``try_empty`` refuses past this (ADVICE
        # r03: a caller keeping a whole clip of results must not pin all of it)
        self.cap_bytes = int(os.environ.get("VF_PINNED_RESULT_CAP", 1 << 30)) if cap_bytes is None else cap_bytes
        self.outstanding = 0
        self.outstanding_bytes = 0

    @staticmethod
    def _cap(nbytes: int) -> int:
        return max(4096, (int(nbytes) + 4095) & ~4095)

    def empty(self, shape, dtype=np.uint8) -> np.ndarray:
        dtype = np.dtype(dtype)
        nbytes = int(np.prod(shape, dtype=np.int64)) * dtype.itemsize
        cap = self._cap(nbytes)
        with self._lock:
            lst = self._free.get(cap)
            ptr = lst.pop() if lst else 0
            if ptr:
                self._free_bytes -= cap
            self.outstanding += 1
            self.outstanding_bytes += cap
        if not ptr:
            try:
                ptr = self._ctx.alloc_host(cap)
            except Exception:
                with self._lock:
                    self.outstanding -= 1
                    self.outstanding_bytes -= cap
                raise
        return np.asarray(_PinnedBlock(self, ptr, cap, shape, dtype))

    def try_empty(self, shape, dtype=np.uint8) -> Optional[np.ndarray]:
        """``empty``, or None when the live result arrays would pass ``cap_bytes`` or the
        page-locked allocation fails (memlock limit, out of memory): the caller then uses
        pageable memory, as ``cv2.bitwise_not`` would."""
        nbytes = int(np.prod(shape, dtype=np.int64)) * np.dtype(dtype).itemsize
        with self._lock:
            if self.outstanding_bytes + self._cap(nbytes) > self.cap_bytes:
                return None
        try:
            return self.empty(shape, dtype)
        except VFilterError:
            return None

    def release(self, ptr: int, cap: int) -> None:
        drop = []
        with self._lock:
            self.outstanding -= 1
            self.outstanding_bytes -= cap
            self._free.setdefault(cap, []).append(ptr)
            self._free_bytes += cap
            while self._free_bytes > self._keep:
                k = max(self._free, key=lambda c: c if self._free[c] else -1)
                drop.append(self._free[k].pop())
                self._free_bytes -= k
            last = self.outstanding == 0
        ctx = self._ctx
        for p in drop:
            ctx._free_host_raw(p)
        if last and ctx._closing:
            _defer_destroy(ctx)  # not here: this runs in a GC finalizer, on any thread

    def drain(self) -> list:
        with self._lock:
            ptrs = [p for lst in self._free.values() for p in lst]
            self._free.clear()
            self._free_bytes = 0
            return ptrs


class Context:
    """One ``vf_ctx``: a device, its HIP streams and the pinned staging ring.

    Mirrors the per-process filter state of ``InverterWorker.__init__`` (inverter.py:10-20);
    one per worker process, bound to one GPU.  Not thread-safe.
    """

    def __init__(self, device: int = 0, max_frame_bytes: int = 0, max_batch: int = 1):
        self._lib = load_library()
        self._closing = False
        self._h = _vp()
        reap_closed_contexts()
        st = self._lib.vf_create(int(device), int(max_frame_bytes), int(max_batch), ctypes.byref(self._h))
        if st != VF_OK:
            raise VFilterError(self._lib.vf_last_error(None).decode(), st, self._lib.vf_last_hip_error(None))
        self.device = int(device)
        self._arena = _PinnedArena(self)
        self._jpeg_n = {}  # ticket -> frame count of every submitted JPEG batch not yet collected

    @property
    def _ctx(self):
        """The library handle for a call; a closed context refuses every call, also while arrays
        of its pinned arena keep its memory alive."""
        if self._closing or not self._h:
            raise VFilterError("vfilter context is closed", VF_E_INVALID, 0)
        return self._h

    # -- plumbing -----------------------------------------------------------------------
    def _check(self, st: int) -> None:
        # the calling thread's own error record: JPEG calls may fail on two threads at once
        # on one context, and the context's record holds whichever failed last
        if st != VF_OK:
            raise VFilterError(self._lib.vf_last_error(None).decode(), st, self._lib.vf_last_hip_error(None))

    @property
    def handle(self) -> int:
        return self._h.value or 0

    @property
    def closed(self) -> bool:
        return self._closing

    def close(self) -> None:
        """Close the context: every later call raises.  The library context is destroyed now,
        or -- while arrays of its pinned arena are alive (their memory must outlive them) --
        at the first ``reap_closed_contexts()`` after the last of them is gone (called by the
        next ``Context()`` and at interpreter exit), never from a garbage-collector finalizer."""
        h = self.__dict__.get("_h")
        if not h:
            return
        self._closing = True
        arena = self.__dict__.get("_arena")
        if arena is not None:
            for p in arena.drain():
                self._free_host_raw(p)
            if arena.outstanding:
                return
        self._destroy()

    def _destroy(self) -> None:
        h = self.__dict__.get("_h")
        if h:
            self._lib.vf_destroy(h)
            self._h = _vp()

    def _free_host_raw(self, p: int) -> None:
        if self._h:
            self._lib.vf_free_host(self._h, p)

    # -- pinned result arrays ------------------------------------------------------------------
    def pinned_empty(self, shape, dtype=np.uint8) -> np.ndarray:
        """An uninitialised array in page-locked, device-mapped memory from the context's arena
        (recycled when the array and its views are gone): the invert kernel writes such a
        destination directly over PCIe, and reads such a source directly."""
        return self._arena.empty(shape, dtype)

    def pinned_empty_like(self, a: np.ndarray) -> np.ndarray:
        return self._arena.empty(a.shape, a.dtype)

    def __enter__(self) -> "Context":
        return self

    def __exit__(self, *exc) -> None:
        self.close()

    def __del__(self):  # best effort
        try:
            self.close()
        except Exception:
            pass

    # -- host -> host -------------------------------------------------------------------
    def invert_host(self, src, dst, nbytes: Optional[int] = None) -> None:
        if nbytes is None:
            nbytes = src.nbytes if isinstance(src, np.ndarray) else len(src)
        self._check(self._lib.vf_invert_host(self._ctx, _addr(src), _addr(dst), nbytes))

    def invert_batch_host(self, src, dst, frame_bytes: int, n: int) -> None:
        self._check(self._lib.vf_invert_batch_host(self._ctx, _addr(src), _addr(dst), frame_bytes, n))

    def invert_frames_host(self, srcs: Sequence, dsts: Sequence, nbytes: Sequence[int]) -> None:
        n = len(srcs)
        if not (len(dsts) == n == len(nbytes)):
            raise ValueError("srcs, dsts and nbytes must have the same length")
        sa = (ctypes.c_void_p * n)(*[_addr(s) for s in srcs])
        da = (ctypes.c_void_p * n)(*[_addr(d) for d in dsts])
        na = (ctypes.c_size_t * n)(*[int(b) for b in nbytes])
        self._check(self._lib.vf_invert_frames_host(self._ctx, sa, da, na, n))

    # -- 256-entry table filter (cv2.LUT): vf_lut_* ---------------------------------------------
    @staticmethod
    def _table(table, channels: int) -> np.ndarray:
        """``table`` (planar bytes, ``filters.as_table``'s first result) as an array to point at."""
        t = np.frombuffer(table, dtype=np.uint8) if not isinstance(table, np.ndarray) else table
        if t.dtype != np.uint8 or t.size != 256 * channels or not t.flags.c_contiguous:
            raise ValueError("table must be channels x 256 contiguous uint8 (see vfilter.as_table)")
        return t

    def lut_frames_host(self, srcs: Sequence, dsts: Sequence, nbytes: Sequence[int], table, channels: int) -> None:
        n = len(srcs)
        if not (len(dsts) == n == len(nbytes)):
            raise ValueError("srcs, dsts and nbytes must have the same length")
        t = self._table(table, channels)
        sa = (ctypes.c_void_p * n)(*[_addr(s) for s in srcs])
        da = (ctypes.c_void_p * n)(*[_addr(d) for d in dsts])
        na = (ctypes.c_size_t * n)(*[int(b) for b in nbytes])
        self._check(self._lib.vf_lut_frames_host(self._ctx, sa, da, na, n, t.ctypes.data, channels))

    def lut_device(self, dsrc: int, ddst: int, nbytes: int, table, channels: int, stream: int = 0) -> None:
        t = self._table(table, channels)
        self._check(self._lib.vf_lut_device(self._ctx, dsrc, ddst, nbytes, t.ctypes.data, channels, stream or None))

    # -- 2-D convolution filter (cv2.filter2D): vf_conv_* ---------------------------------------
    @staticmethod
    def _weights(weights) -> np.ndarray:
        """``weights`` (``filters.as_kernel``'s first result) as an array to point at."""
        w = np.asarray(weights)
        if w.dtype != np.int16 or w.ndim != 2 or not w.flags.c_contiguous:
            raise ValueError("weights must be a C-contiguous kh x kw int16 array (see vfilter.as_kernel)")
        return w

    @staticmethod
    def _frame_arrays(srcs: Sequence, dsts: Sequence, widths: Sequence[int], heights: Sequence[int]):
        """The pointer and size arrays of a ``*_frames_host`` call over shaped frames, and their length."""
        n = len(srcs)
        if not (len(dsts) == n == len(widths) == len(heights)):
            raise ValueError("srcs, dsts, widths and heights must have the same length")
        sa = (ctypes.c_void_p * n)(*[_addr(s) for s in srcs])
        da = (ctypes.c_void_p * n)(*[_addr(d) for d in dsts])
        wa = (ctypes.c_int * n)(*[int(v) for v in widths])
        ha = (ctypes.c_int * n)(*[int(v) for v in heights])
        return sa, da, wa, ha, n

    def conv_frames_host(self, srcs: Sequence, dsts: Sequence, widths: Sequence[int], heights: Sequence[int],
                         channels: int, weights, shift: int, border: int = 0) -> None:
        sa, da, wa, ha, n = self._frame_arrays(srcs, dsts, widths, heights)
        w = self._weights(weights)
        self._check(self._lib.vf_conv_frames_host(self._ctx, sa, da, wa, ha, n, channels, w.ctypes.data, w.shape[1],
                                                  w.shape[0], shift, border))

    def conv_device(self, dsrc: int, ddst: int, width: int, height: int, channels: int, weights, shift: int,
                    border: int = 0, stream: int = 0) -> None:
        w = self._weights(weights)
        self._check(self._lib.vf_conv_device(self._ctx, dsrc, ddst, width, height, channels, w.ctypes.data, w.shape[1],
                                             w.shape[0], shift, border, stream or None))

    # -- rank filters (cv2.erode, cv2.dilate, cv2.medianBlur): vf_rank_* ----------------------------
    @staticmethod
    def _element(element) -> np.ndarray:
        """``element`` (``filters.as_element``'s result) as an array to point at."""
        e = np.asarray(element)
        if e.dtype != np.uint8 or e.ndim != 2 or not e.flags.c_contiguous:
            raise ValueError("element must be a C-contiguous kh x kw uint8 array (see vfilter.as_element)")
        return e

    def rank_frames_host(self, srcs: Sequence, dsts: Sequence, widths: Sequence[int], heights: Sequence[int],
                         channels: int, op: int, element, border: int = 2) -> None:
        sa, da, wa, ha, n = self._frame_arrays(srcs, dsts, widths, heights)
        e = self._element(element)
        self._check(self._lib.vf_rank_frames_host(self._ctx, sa, da, wa, ha, n, channels, op, e.ctypes.data, e.shape[1],
                                                  e.shape[0], border))

    def rank_device(self, dsrc: int, ddst: int, width: int, height: int, channels: int, op: int, element,
                    border: int = 2, stream: int = 0) -> None:
        e = self._element(element)
        self._check(self._lib.vf_rank_device(self._ctx, dsrc, ddst, width, height, channels, op, e.ctypes.data,
                                             e.shape[1], e.shape[0], border, stream or None))

    # -- colour matrix (cv2.transform): vf_mix_* ------------------------------------------------------
    @staticmethod
    def _matrix(matrix) -> np.ndarray:
        """``matrix`` (``filters.as_matrix``'s first result) as an array to point at."""
        m = np.asarray(matrix)
        if m.dtype != np.int32 or m.shape != (3, 4) or not m.flags.c_contiguous:
            raise ValueError("matrix must be a C-contiguous 3 x 4 int32 array (see vfilter.as_matrix)")
        return m

    def mix_tile_bytes(self) -> int:
        """The bytes of one workgroup's tile of the colour-matrix kernel."""
        return int(self._lib.vf_mix_tile_bytes())

    def mix_frames_host(self, srcs: Sequence, dsts: Sequence, widths: Sequence[int], heights: Sequence[int],
                        channels: int, matrix, shift: int, rounding: int = 0) -> None:
        sa, da, wa, ha, n = self._frame_arrays(srcs, dsts, widths, heights)
        m = self._matrix(matrix)
        self._check(self._lib.vf_mix_frames_host(self._ctx, sa, da, wa, ha, n, channels, m.ctypes.data, shift, rounding))

    def mix_device(self, dsrc: int, ddst: int, nbytes: int, matrix, shift: int, rounding: int = 0,
                   stream: int = 0) -> None:
        """The matrix over ``nbytes`` of device memory (whole 3-byte pixels); asynchronous."""
        m = self._matrix(matrix)
        self._check(self._lib.vf_mix_device(self._ctx, dsrc or None, ddst or None, nbytes, m.ctypes.data, shift,
                                            rounding, stream or None))

    # -- separable filter (cv2.sepFilter2D, cv2.blur, cv2.boxFilter): vf_sep_* ------------------------------
    @staticmethod
    def _taps(taps) -> np.ndarray:
        """``taps`` (``filters.as_taps``'s first result) as an array to point at."""
        t = np.asarray(taps)
        if t.dtype != np.int16 or t.ndim != 1 or not t.flags.c_contiguous:
            raise ValueError("taps must be a C-contiguous 1-D int16 array (see vfilter.as_taps)")
        return t

    def sep_tile(self, kw: int, kh: int) -> tuple:
        """``(row_bytes, rows)`` of one workgroup's output tile of the separable kernel for kw x kh taps."""
        rb, rows = ctypes.c_int(0), ctypes.c_int(0)
        if self._lib.vf_sep_tile(kw, kh, ctypes.byref(rb), ctypes.byref(rows)) != 0:
            raise ValueError(f"sep_tile: tap counts {kw} x {kh}; they are odd and at most 31")
        return rb.value, rows.value

    def sep_frames_host(self, srcs: Sequence, dsts: Sequence, widths: Sequence[int], heights: Sequence[int],
                        channels: int, kx, ky, shift: int = 0, divisor: int = 1, rounding: int = 0,
                        border: int = 0) -> None:
        sa, da, wa, ha, n = self._frame_arrays(srcs, dsts, widths, heights)
        x, y = self._taps(kx), self._taps(ky)
        self._check(self._lib.vf_sep_frames_host(self._ctx, sa, da, wa, ha, n, channels, x.ctypes.data, x.size,
                                                 y.ctypes.data, y.size, shift, divisor, rounding, border))

    def sep_device(self, dsrc: int, ddst: int, width: int, height: int, channels: int, kx, ky, shift: int = 0,
                   divisor: int = 1, rounding: int = 0, border: int = 0, stream: int = 0) -> None:
        x, y = self._taps(kx), self._taps(ky)
        self._check(self._lib.vf_sep_device(self._ctx, dsrc, ddst, width, height, channels, x.ctypes.data, x.size,
                                            y.ctypes.data, y.size, shift, divisor, rounding, border, stream or None))

    # -- level filter (cv2.equalizeHist, auto-levels) and the histogram: vf_hist_*, vf_level_* ----------------
    def hist_frames_host(self, srcs: Sequence, channels: int, hists: np.ndarray) -> None:
        """The histograms of the frames ``srcs`` (``channels`` interleaved channels each, mixed sizes) into ``hists``,
        a C-contiguous uint32 array of ``len(srcs) * channels * 256`` entries."""
        n = len(srcs)
        if hists.dtype != np.uint32 or not hists.flags.c_contiguous or hists.size != n * channels * 256:
            raise ValueError("hists must be a C-contiguous uint32 array of len(srcs) * channels * 256 entries")
        keep = [np.ascontiguousarray(s) for s in srcs]
        sa = (ctypes.c_void_p * n)(*[_addr(s) if s.size else None for s in keep])
        na = (ctypes.c_size_t * n)(*[int(s.nbytes) for s in keep])
        self._check(self._lib.vf_hist_frames_host(self._ctx, sa, na, n, channels, hists.ctypes.data))

    def hist_device(self, dsrc: int, nbytes: int, channels: int, dhist: int, stream: int = 0) -> None:
        self._check(self._lib.vf_hist_device(self._ctx, dsrc or None, nbytes, channels, dhist or None, stream or None))

    def level_frames_host(self, srcs: Sequence, dsts: Sequence, widths: Sequence[int], heights: Sequence[int],
                          channels: int, rule: int, mask: int = 0, link: int = 0, clip_lo: int = 0,
                          clip_hi: int = 0) -> None:
        sa, da, wa, ha, n = self._frame_arrays(srcs, dsts, widths, heights)
        self._check(self._lib.vf_level_frames_host(self._ctx, sa, da, wa, ha, n, channels, rule, mask, link, clip_lo,
                                                   clip_hi))

    def level_device(self, dsrc: int, ddst: int, width: int, height: int, channels: int, rule: int, mask: int = 0,
                     link: int = 0, clip_lo: int = 0, clip_hi: int = 0, stream: int = 0) -> None:
        self._check(self._lib.vf_level_device(self._ctx, dsrc or None, ddst or None, width, height, channels, rule, mask,
                                              link, clip_lo, clip_hi, stream or None))

    # -- CLAHE (cv2.createCLAHE(...).apply): vf_clahe_* ------------------------------------------------------
    def clahe_frames_host(self, srcs: Sequence, dsts: Sequence, widths: Sequence[int], heights: Sequence[int],
                          channels: int, clip_q8: int, tiles_x: int = 8, tiles_y: int = 8, mask: int = 0) -> None:
        sa, da, wa, ha, n = self._frame_arrays(srcs, dsts, widths, heights)
        self._check(self._lib.vf_clahe_frames_host(self._ctx, sa, da, wa, ha, n, channels, clip_q8, tiles_x, tiles_y, mask))

    def clahe_device(self, dsrc: int, ddst: int, width: int, height: int, channels: int, clip_q8: int, tiles_x: int = 8,
                     tiles_y: int = 8, mask: int = 0, stream: int = 0) -> None:
        self._check(self._lib.vf_clahe_device(self._ctx, dsrc or None, ddst or None, width, height, channels, clip_q8,
                                              tiles_x, tiles_y, mask, stream or None))

    # -- the affine warp (cv2.warpAffine, cv2.flip): vf_warp_* -----------------------------------------------
    @staticmethod
    def _warp_args(m, mode: int, interp: int, border: int, value) -> tuple:
        """``filters.Warp.args`` as the C arguments ``(m, mode, interp, border, value)``: six doubles and three ints."""
        mm = (ctypes.c_double * 6)(*([float(v) for v in m] if m is not None else [0.0] * 6))
        vv = (ctypes.c_int * 3)(*[int(v) for v in value])
        return mm, int(mode), int(interp), int(border), vv

    def warp_frames_host(self, srcs: Sequence, dsts: Sequence, widths: Sequence[int], heights: Sequence[int],
                         channels: int, m, mode: int = 0, interp: int = 0, border: int = 2, value=(0, 0, 0)) -> None:
        sa, da, wa, ha, n = self._frame_arrays(srcs, dsts, widths, heights)
        self._check(self._lib.vf_warp_frames_host(self._ctx, sa, da, wa, ha, n, channels,
                                                  *self._warp_args(m, mode, interp, border, value)))

    def warp_device(self, dsrc: int, ddst: int, width: int, height: int, channels: int, m, mode: int = 0,
                    interp: int = 0, border: int = 2, value=(0, 0, 0), stream: int = 0) -> None:
        self._check(self._lib.vf_warp_device(self._ctx, dsrc or None, ddst or None, width, height, channels,
                                             *self._warp_args(m, mode, interp, border, value), stream or None))

    # -- the resize (cv2.resize): vf_resize_* ----------------------------------------------------------------
    def resize_out_size(self, width: int, height: int, dw: int = 0, dh: int = 0, fx: float = 0.0, fy: float = 0.0,
                        interp: int = INTER_LINEAR) -> tuple:
        """``(width, height)`` of the result for a frame of ``width`` x ``height``."""
        ow, oh = ctypes.c_int(0), ctypes.c_int(0)
        self._check(self._lib.vf_resize_out_size(self._ctx, width, height, int(dw), int(dh), float(fx), float(fy),
                                                 int(interp), ctypes.byref(ow), ctypes.byref(oh)))
        return ow.value, oh.value

    def resize_frames_host(self, srcs: Sequence, dsts: Sequence, widths: Sequence[int], heights: Sequence[int],
                           channels: int, dw: int = 0, dh: int = 0, fx: float = 0.0, fy: float = 0.0,
                           interp: int = INTER_LINEAR) -> None:
        """``dsts[i]`` holds frame i's result size (``resize_out_size``)."""
        sa, da, wa, ha, n = self._frame_arrays(srcs, dsts, widths, heights)
        self._check(self._lib.vf_resize_frames_host(self._ctx, sa, da, wa, ha, n, channels, int(dw), int(dh), float(fx),
                                                    float(fy), int(interp)))

    def resize_device(self, dsrc: int, ddst: int, width: int, height: int, channels: int, dw: int = 0, dh: int = 0,
                      fx: float = 0.0, fy: float = 0.0, interp: int = INTER_LINEAR, stream: int = 0) -> None:
        self._check(self._lib.vf_resize_device(self._ctx, dsrc or None, ddst or None, width, height, channels, int(dw),
                                               int(dh), float(fx), float(fy), int(interp), stream or None))

    # -- filter chains (vf_chain_*, vf_binary_device) ------------------------------------------------
    def _steps(self, steps: Sequence):
        """``steps`` -- ``filters.Chain.args[0]``: tuples ``(kind, a, b, op, data, shift, border)`` with
        ``data`` the planar table bytes, the int16 weights, the element, the int32 matrix or ``None`` -- as a ``vf_step``
        array, with the arrays it points at (keep both alive across the call)."""
        arr = (Step * max(len(steps), 1))()
        keep = []
        for st, (kind, a, b, op, data, shift, border) in zip(arr, steps):
            st.kind, st.a, st.b, st.op, st.shift, st.border = kind, a, b, op, shift, border
            if kind == STEP_TABLE:
                st.channels = len(data) // 256
                d = self._table(data, st.channels)
            elif kind == STEP_CONV:
                d = self._weights(data)
                st.kh, st.kw = d.shape
            elif kind == STEP_RANK:
                d = self._element(data)
                st.kh, st.kw = d.shape
            elif kind == STEP_MIX:
                d = self._matrix(data)
            elif kind == STEP_SEP:  # data: (kx, ky, divisor) -> the divisor, kx, ky as int32
                kx, ky, divisor = data
                st.kw, st.kh = len(kx), len(ky)
                d = np.concatenate([[divisor], self._taps(kx), self._taps(ky)]).astype(np.int32)
            elif kind == STEP_LEVEL:  # data: (mask, link, clip_lo, clip_hi); op: the rule
                d = np.array([int(v) for v in data], np.int32)
                if d.shape != (4,):
                    raise ValueError("a level step's data is (mask, link, clip_lo, clip_hi)")
            elif kind == STEP_CLAHE:  # data: (mask, clip_q8, tiles_x, tiles_y)
                d = np.array([int(v) for v in data], np.int32)
                if d.shape != (4,):
                    raise ValueError("a CLAHE step's data is (mask, clip_q8, tiles_x, tiles_y)")
            elif kind == STEP_WARP:  # data: (m, mode, interp, value) -> six float64, then six int32
                m, mode, interp, value = data
                ints = np.array([int(mode), int(interp)] + [int(v) for v in value] + [0], np.int32)
                d = np.frombuffer(np.array([float(v) for v in m], np.float64).tobytes() + ints.tobytes(), np.uint8)
                if d.shape != (72,):
                    raise ValueError("a warp step's data is (the six entries of m, mode, interp, the three border bytes)")
            elif kind == STEP_RESIZE:  # data: (dw, dh, fx, fy, interp) -> two float64, then four int32
                dw, dh, fx, fy, interp = data
                ints = np.array([int(dw), int(dh), int(interp), 0], np.int32)
                d = np.frombuffer(np.array([float(fx), float(fy)], np.float64).tobytes() + ints.tobytes(), np.uint8)
            else:
                d = None
            if d is not None:
                keep.append(d)
                st.data = d.ctypes.data
        return arr, keep

    def chain_frames_host(self, srcs: Sequence, dsts: Sequence, widths: Sequence[int], heights: Sequence[int],
                          channels: int, steps: Sequence) -> None:
        sa, da, wa, ha, n = self._frame_arrays(srcs, dsts, widths, heights)
        arr, keep = self._steps(steps)
        self._check(self._lib.vf_chain_frames_host(self._ctx, sa, da, wa, ha, n, channels, arr, len(steps)))
        del keep

    def chain_out_size(self, steps: Sequence, channels: int, width: int, height: int) -> tuple:
        """``(width, height)`` of the program's result for a frame of ``width`` x ``height``."""
        arr, keep = self._steps(steps)
        ow, oh = ctypes.c_int(0), ctypes.c_int(0)
        self._check(self._lib.vf_chain_out_size(self._ctx, arr, len(steps), channels, width, height, ctypes.byref(ow),
                                                ctypes.byref(oh)))
        del keep
        return ow.value, oh.value

    def binary_device(self, da: int, db: int, ddst: int, nbytes: int, op: int, stream: int = 0) -> None:
        """``ddst[i] = op(da[i], db[i])`` over device memory, ``op`` a ``VF_BIN_*``; asynchronous."""
        self._check(self._lib.vf_binary_device(self._ctx, da or None, db or None, ddst or None, nbytes, op,
                                               stream or None))

    # -- host -> host, asynchronous (page-locked buffers) -----------------------------------
    def invert_frames_async(self, srcs: Sequence, dsts: Sequence, nbytes: Sequence[int]) -> int:
        """Enqueue a batch whose buffers are all page-locked; returns a ticket for ``wait``.
        The caller keeps the buffers alive until the ticket completes."""
        n = len(srcs)
        if not (len(dsts) == n == len(nbytes)):
            raise ValueError("srcs, dsts and nbytes must have the same length")
        sa = (ctypes.c_void_p * n)(*[_addr(s) for s in srcs])
        da = (ctypes.c_void_p * n)(*[_addr(d) for d in dsts])
        na = (ctypes.c_size_t * n)(*[int(b) for b in nbytes])
        t = ctypes.c_uint64(0)
        self._check(self._lib.vf_invert_frames_async(self._ctx, sa, da, na, n, ctypes.byref(t)))
        return t.value

    def invert_frames_async_addrs(self, src_addrs: np.ndarray, dst_addrs: np.ndarray, nbytes: np.ndarray) -> int:
        """``invert_frames_async`` from address arrays (a worker's ring slots: base + slot
        arithmetic, no ndarray per frame; ``ndarray.ctypes`` costs ~2.5 us an access)."""
        sa = np.ascontiguousarray(src_addrs, np.uint64)
        da = np.ascontiguousarray(dst_addrs, np.uint64)
        na = np.ascontiguousarray(nbytes, np.uint64)
        n = len(sa)
        if not (len(da) == n == len(na)):
            raise ValueError("srcs, dsts and nbytes must have the same length")
        t = ctypes.c_uint64(0)
        self._check(self._lib.vf_invert_frames_async(self._ctx, sa.ctypes.data, da.ctypes.data, na.ctypes.data, n,
                                                     ctypes.byref(t)))
        return t.value

    def wait(self, ticket: int) -> float:
        """Block until ``ticket`` completes; returns its device time in ms (-1 if unknown)."""
        ms = ctypes.c_float(-1.0)
        self._check(self._lib.vf_wait(self._ctx, ticket, ctypes.byref(ms)))
        return ms.value

    def query(self, ticket: int) -> bool:
        done = ctypes.c_int(0)
        self._check(self._lib.vf_query(self._ctx, ticket, ctypes.byref(done)))
        return bool(done.value)

    # -- device-resident ------------------------------------------------------------------
    def invert_device(self, dsrc: int, ddst: int, nbytes: int, stream: int = 0) -> None:
        self._check(self._lib.vf_invert_device(self._ctx, dsrc, ddst, nbytes, stream or None))

    def invert_device_frames(self, dsrcs_dev: int, ddsts_dev: int, nbytes_dev: int, n: int,
                             total_bytes: int, stream: int = 0) -> None:
        self._check(self._lib.vf_invert_device_frames(self._ctx, dsrcs_dev, ddsts_dev, nbytes_dev, n,
                                                      total_bytes, stream or None))

    def alloc_device(self, nbytes: int) -> int:
        p = _vp()
        self._check(self._lib.vf_alloc_device(self._ctx, nbytes, ctypes.byref(p)))
        return p.value or 0

    def free_device(self, p: int) -> None:
        self._check(self._lib.vf_free_device(self._ctx, p))

    def alloc_host(self, nbytes: int) -> int:
        p = _vp()
        self._check(self._lib.vf_alloc_host(self._ctx, nbytes, ctypes.byref(p)))
        return p.value or 0

    def free_host(self, p: int) -> None:
        self._check(self._lib.vf_free_host(self._ctx, p))

    def host_register(self, buf, nbytes: Optional[int] = None) -> int:
        addr = _addr(buf)
        if nbytes is None:
            nbytes = buf.nbytes if isinstance(buf, np.ndarray) else len(buf)
        self._check(self._lib.vf_host_register(self._ctx, addr, nbytes))
        return addr

    def host_unregister(self, addr: int) -> None:
        self._check(self._lib.vf_host_unregister(self._ctx, addr))

    def upload(self, ddst: int, hsrc, nbytes: int, stream: int = 0) -> None:
        self._check(self._lib.vf_upload(self._ctx, ddst, _addr(hsrc), nbytes, stream or None))

    def download(self, hdst, dsrc: int, nbytes: int, stream: int = 0) -> None:
        self._check(self._lib.vf_download(self._ctx, _addr(hdst), dsrc, nbytes, stream or None))

    def memset_device(self, d: int, value: int, nbytes: int, stream: int = 0) -> None:
        self._check(self._lib.vf_memset_device(self._ctx, d, value, nbytes, stream or None))

    def sync(self, stream: int = 0) -> None:
        self._check(self._lib.vf_sync(self._ctx, stream or None))

    def elapsed_ms(self) -> float:
        ms = ctypes.c_float(0.0)
        self._check(self._lib.vf_elapsed_ms(self._ctx, ctypes.byref(ms)))
        return ms.value

    def last_timeline(self) -> list:
        """[(bytes, h2d_start_ms, kernel_start_ms, kernel_end_ms, d2h_end_ms), ...] per chunk
        of the last host->host call, ms after the call's start event."""
        n = ctypes.c_int(0)
        self._check(self._lib.vf_last_timeline(self._ctx, None, None, 0, ctypes.byref(n)))
        if n.value == 0:
            return []
        out = (ctypes.c_float * (4 * n.value))()
        nb = (ctypes.c_size_t * n.value)()
        self._check(self._lib.vf_last_timeline(self._ctx, out, nb, n.value, ctypes.byref(n)))
        return [(int(nb[i]),) + tuple(float(out[4 * i + j]) for j in range(4)) for i in range(n.value)]

    def bench_device_ring(self, srcs: Sequence[int], dsts: Sequence[int], nbytes: int, steps: int,
                          stream: int = 0, per_launch: bool = False):
        """Launch ``steps`` kernels back to back over the ring; returns (region_ms,
        per-launch ms array or None).  See vf_bench_device_ring."""
        nbuf = len(srcs)
        sa = (ctypes.c_void_p * nbuf)(*srcs)
        da = (ctypes.c_void_p * nbuf)(*dsts)
        out = np.zeros(max(steps, 1), dtype=np.float32) if per_launch else None
        region = ctypes.c_float(0.0)
        self._check(self._lib.vf_bench_device_ring(
            self._ctx, sa, da, nbuf, nbytes, steps, stream or None,
            out.ctypes.data_as(_c_float_p) if per_launch else None, ctypes.byref(region)))
        return region.value, (out[:steps] if per_launch else None)


    # -- JPEG (default use_jpeg=True mode: inverter.py:32 -> :41 -> :44) -----------------------
    def _out_arena(self, caps: Sequence[int]) -> list:
        """Per-frame output windows (worst-case tjBufSize each) in one grow-only host arena
        reused across calls: the encoder writes only the few hundred KB each JPEG needs, and
        reused pages take no page faults.  Results are copied out (bytes) before returning."""
        offs, tot = [], 0
        for c in caps:
            offs.append(tot)
            tot += (int(c) + 63) & ~63
        tls = self.__dict__.setdefault("_arena_tls", threading.local())  # one arena per calling thread
        arena = getattr(tls, "arena", None)
        if arena is None or arena.nbytes < tot:
            arena = tls.arena = np.empty(tot, np.uint8)
        return [arena[o:o + c] for o, c in zip(offs, caps)]

    @staticmethod
    def _ptrs(bufs):
        arrs = [b if isinstance(b, np.ndarray) else np.frombuffer(b, dtype=np.uint8) for b in bufs]
        return arrs, (ctypes.c_void_p * len(arrs))(*[a.ctypes.data for a in arrs])

    def jpeg_set_max_pixels(self, max_pixels: int) -> None:
        """Decoder frame-size limit (vf_jpeg_set_max_pixels; 0 = the default, 8192 x 8192)."""
        self._check(self._lib.vf_jpeg_set_max_pixels(self._ctx, int(max_pixels)))

    def jpeg_encode(self, imgs: Sequence[np.ndarray], pixel_format: int, quality: int, subsamp: int,
                    flags: int = 0) -> list:
        """Encode H x W x 3 uint8 images in one batched GPU pass; returns a list of bytes."""
        n = len(imgs)
        if n == 0:
            return []
        imgs = [np.ascontiguousarray(a, dtype=np.uint8) for a in imgs]
        for a in imgs:
            if a.ndim != 3 or a.shape[2] != 3:
                raise ValueError("jpeg_encode: images must be H x W x 3 uint8")
        _, ia = self._ptrs(imgs)
        ws = (ctypes.c_int * n)(*[a.shape[1] for a in imgs])
        hs = (ctypes.c_int * n)(*[a.shape[0] for a in imgs])
        caps = [int(self._lib.vf_jpeg_buffer_size(a.shape[1], a.shape[0], subsamp)) for a in imgs]
        if not all(caps):
            raise ValueError("jpeg_encode: unsupported size or subsampling")
        outs = self._out_arena(caps)
        _, oa = self._ptrs(outs)
        ca = (ctypes.c_size_t * n)(*caps)
        sz = (ctypes.c_size_t * n)()
        self._check(self._lib.vf_jpeg_encode(self._ctx, ia, ws, hs, n, pixel_format, quality, subsamp, flags,
                                             oa, ca, sz))
        return [outs[i][:sz[i]].tobytes() for i in range(n)]

    def jpeg_decode(self, jpegs: Sequence, pixel_format: int, flags: int = 0) -> list:
        """Decode JPEGs in one batched GPU pass; returns H x W x 3 uint8 arrays."""
        n = len(jpegs)
        if n == 0:
            return []
        srcs, ja = self._ptrs(jpegs)
        outs = []
        for s in srcs:
            w, h, _, _ = jpeg_header(s)
            outs.append(np.empty((h, w, 3), np.uint8))
        _, oa = self._ptrs(outs)
        js = (ctypes.c_size_t * n)(*[s.nbytes for s in srcs])
        ca = (ctypes.c_size_t * n)(*[o.nbytes for o in outs])
        self._check(self._lib.vf_jpeg_decode(self._ctx, ja, js, n, pixel_format, flags, oa, ca))
        return outs

    # The JPEG filters differ in one C function each and in the arguments that stand between the
    # batch and the quality, ``extra`` below: none (invert), ``table, channels`` (lut), ``weights, kw,
    # kh, shift, border`` (conv), ``op, element, kw, kh, border`` (rank).  The pointers keep their
    # arrays alive (``data_as``).
    def _table_args(self, table, channels: int) -> tuple:
        return self._table(table, channels).ctypes.data_as(_vp), channels

    def _weights_args(self, weights, shift: int, border: int) -> tuple:
        w = self._weights(weights)
        return w.ctypes.data_as(_vp), w.shape[1], w.shape[0], shift, border

    def _element_args(self, op: int, element, border: int) -> tuple:
        e = self._element(element)
        return op, e.ctypes.data_as(_vp), e.shape[1], e.shape[0], border

    def _jpeg_submit(self, name: str, fn, extra, jpegs, sizes, quality: int, subsamp: int, flags: int) -> int:
        """Every ``jpeg_*_submit*``: stage the batch through ``fn`` and note its frame count under the
        ticket.  ``sizes`` None: ``jpegs`` is a list of buffers; else ``jpegs`` and ``sizes`` are address
        and size arrays (the JPEGs in a worker's ring slots)."""
        if sizes is None:
            n = len(jpegs)
            if n == 0:
                raise ValueError(f"{name}: empty batch")
            srcs, ja = self._ptrs(jpegs)
            js = (ctypes.c_size_t * n)(*[s.nbytes for s in srcs])
        else:
            a = np.ascontiguousarray(jpegs, np.uint64)
            z = np.ascontiguousarray(sizes, np.uint64)
            n = len(a)
            if n == 0 or len(z) != n:
                raise ValueError(f"{name}: empty batch or sizes of another length")
            ja, js = a.ctypes.data, z.ctypes.data
        t = ctypes.c_uint64(0)
        self._check(fn(self._ctx, ja, js, n, *extra, quality, subsamp, flags, ctypes.byref(t)))
        self._jpeg_n[t.value] = n
        return t.value

    def _jpeg_bench(self, fn, extra, colour: str, jpegs: Sequence, quality: int, subsamp: int, flags: int, iters: int):
        """Every ``jpeg_bench_*``; ``colour``: the filter's name for the colour stage."""
        n = len(jpegs)
        srcs, ja = self._ptrs(jpegs)
        js = (ctypes.c_size_t * n)(*[s.nbytes for s in srcs])
        ms = ctypes.c_float(0)
        st = (ctypes.c_float * 8)()
        self._check(fn(self._ctx, ja, js, n, *extra, quality, subsamp, flags, iters, ctypes.byref(ms), st))
        names = ("unstuff", "huffman_sync", "huffman_write", "dc_idct", colour, "fdct_huffman",
                 "stuffing", "sync_passes")
        return ms.value, dict(zip(names, [float(x) for x in st]))

    def _jpeg_take(self, ticket: int, name: str = "", outputs: Optional[int] = None) -> int:
        """The frame count of a submitted batch, taken off the table; ``outputs`` (how many the caller
        brought), when given, must equal it, else the ticket stays collectable."""
        n = self._jpeg_n.pop(ticket, None)
        if n is None:
            raise VFilterError(f"unknown JPEG ticket {ticket}", VF_E_INVALID)
        if outputs is not None and outputs != n:
            self._jpeg_n[ticket] = n
            raise ValueError(f"{name}: {outputs} outputs for a batch of {n}")
        return n

    def jpeg_invert(self, jpegs: Sequence, quality: int, subsamp: int, flags: int = 0) -> list:
        """decode -> bitwise_not -> encode for every JPEG, fused on the GPU; returns bytes."""
        if len(jpegs) == 0:
            return []
        return [v.tobytes() for v in self.jpeg_invert_result(self.jpeg_invert_submit(jpegs, quality, subsamp, flags))]

    # -- the same, asynchronously: submit now, collect later (vf_jpeg_invert_submit & co.) ---------
    def jpeg_invert_submit(self, jpegs: Sequence, quality: int, subsamp: int, flags: int = 0) -> int:
        """Stage the batch and queue its GPU work; returns a ticket at once (the inputs may be
        released as soon as this returns)."""
        return self._jpeg_submit("jpeg_invert_submit", self._lib.vf_jpeg_invert_submit, (), jpegs, None,
                                 quality, subsamp, flags)

    def jpeg_invert_ready(self, ticket: int) -> bool:
        done = ctypes.c_int(0)
        self._check(self._lib.vf_jpeg_invert_query(self._ctx, ticket, ctypes.byref(done)))
        return bool(done.value)

    def jpeg_invert_result(self, ticket: int) -> list:
        """Wait for a submitted batch; returns one uint8 array view per frame, all views into
        one fresh buffer (bytes-like: they can go on the wire as they are)."""
        n = self._jpeg_take(ticket)
        total = ctypes.c_size_t(0)
        self._check(self._lib.vf_jpeg_invert_wait(self._ctx, ticket, ctypes.byref(total)))
        buf = np.empty(max(1, total.value), np.uint8)
        sz = (ctypes.c_size_t * n)()
        off = (ctypes.c_size_t * n)()
        self._check(self._lib.vf_jpeg_invert_fetch(self._ctx, ticket, buf.ctypes.data, buf.nbytes, sz, off))
        return [buf[off[i]:off[i] + sz[i]] for i in range(n)]

    def jpeg_invert_result_into(self, ticket: int, outs: Sequence) -> list:
        """Wait for a submitted batch and write frame i's JPEG into ``outs[i]`` (a writable uint8
        array, e.g. the output half of the frame's ring slot) when it fits; returns per frame a
        view ``outs[i][:size]``, or, for a frame without room (or ``outs[i]`` None), a view into
        one fresh buffer holding it (vf_jpeg_invert_scatter, then a packed fetch only if needed)."""
        n = self._jpeg_take(ticket, "jpeg_invert_result_into", len(outs))
        total = ctypes.c_size_t(0)
        self._check(self._lib.vf_jpeg_invert_wait(self._ctx, ticket, ctypes.byref(total)))
        op = (ctypes.c_void_p * n)(*[None if o is None else o.ctypes.data for o in outs])
        caps = (ctypes.c_size_t * n)(*[0 if o is None else o.nbytes for o in outs])
        sz = (ctypes.c_size_t * n)()
        placed = ctypes.c_int(0)
        try:
            self._check(self._lib.vf_jpeg_invert_scatter(self._ctx, ticket, op, caps, sz, ctypes.byref(placed)))
        except Exception:
            self._lib.vf_jpeg_invert_fetch(self._ctx, ticket, None, 0, None, None)
            raise
        res = [outs[i][:sz[i]] if outs[i] is not None and sz[i] <= caps[i] else None for i in range(n)]
        if placed.value == n:
            self._check(self._lib.vf_jpeg_invert_fetch(self._ctx, ticket, None, 0, None, None))
            return res
        buf = np.empty(max(1, total.value), np.uint8)
        off = (ctypes.c_size_t * n)()
        self._check(self._lib.vf_jpeg_invert_fetch(self._ctx, ticket, buf.ctypes.data, buf.nbytes, sz, off))
        return [r if r is not None else buf[off[i]:off[i] + sz[i]] for i, r in enumerate(res)]

    def jpeg_invert_submit_addrs(self, addrs: np.ndarray, sizes: np.ndarray, quality: int, subsamp: int,
                                 flags: int = 0) -> int:
        """``jpeg_invert_submit`` from address / size arrays (the JPEGs in a worker's ring slots)."""
        return self._jpeg_submit("jpeg_invert_submit_addrs", self._lib.vf_jpeg_invert_submit, (), addrs, sizes,
                                 quality, subsamp, flags)

    def jpeg_invert_result_into_addrs(self, ticket: int, out_addrs: np.ndarray, cap: int):
        """``jpeg_invert_result_into`` for outputs given as addresses of ``cap`` writable bytes each
        (the output halves of ring slots): returns (sizes int64, {i: JPEG} for the frames that did
        not fit and come back in a fresh buffer)."""
        oa = np.ascontiguousarray(out_addrs, np.uint64)
        n = self._jpeg_take(ticket, "jpeg_invert_result_into_addrs", len(oa))
        total = ctypes.c_size_t(0)
        self._check(self._lib.vf_jpeg_invert_wait(self._ctx, ticket, ctypes.byref(total)))
        caps = np.full(n, cap, np.uint64)
        sz = np.zeros(n, np.uint64)
        placed = ctypes.c_int(0)
        try:
            self._check(self._lib.vf_jpeg_invert_scatter(self._ctx, ticket, oa.ctypes.data, caps.ctypes.data,
                                                         sz.ctypes.data, ctypes.byref(placed)))
        except Exception:
            self._lib.vf_jpeg_invert_fetch(self._ctx, ticket, None, 0, None, None)
            raise
        over = {}
        if placed.value == n:
            self._check(self._lib.vf_jpeg_invert_fetch(self._ctx, ticket, None, 0, None, None))
        else:
            buf = np.empty(max(1, total.value), np.uint8)
            off = (ctypes.c_size_t * n)()
            sz2 = (ctypes.c_size_t * n)()
            self._check(self._lib.vf_jpeg_invert_fetch(self._ctx, ticket, buf.ctypes.data, buf.nbytes, sz2, off))
            for i in np.flatnonzero(sz > caps).tolist():
                over[i] = buf[off[i]:off[i] + sz2[i]]
        return sz.astype(np.int64), over

    def jpeg_invert_release(self, ticket: int) -> None:
        """Drop a submitted batch without reading it."""
        if self._jpeg_n.pop(ticket, None) is not None:
            self._check(self._lib.vf_jpeg_invert_fetch(self._ctx, ticket, None, 0, None, None))

    def jpeg_bench_invert(self, jpegs: Sequence, quality: int, subsamp: int, flags: int = 0, iters: int = 10):
        """(mean ms per batch, {stage: ms}) for the GPU part of jpeg_invert on resident inputs."""
        return self._jpeg_bench(self._lib.vf_jpeg_bench_invert, (), "color_invert", jpegs, quality, subsamp, flags,
                                iters)

    # -- JPEG with a table in place of the inversion (vf_jpeg_lut*); tickets are invert tickets ----
    def jpeg_lut(self, jpegs: Sequence, table, channels: int, quality: int, subsamp: int, flags: int = 0) -> list:
        """decode -> cv2.LUT -> encode for every JPEG, fused on the GPU; returns bytes."""
        if len(jpegs) == 0:
            return []
        ticket = self.jpeg_lut_submit(jpegs, table, channels, quality, subsamp, flags)
        return [v.tobytes() for v in self.jpeg_invert_result(ticket)]

    def jpeg_lut_submit(self, jpegs: Sequence, table, channels: int, quality: int, subsamp: int,
                        flags: int = 0) -> int:
        """``jpeg_invert_submit`` with the table; collect with the ``jpeg_invert_result*`` methods."""
        return self._jpeg_submit("jpeg_lut_submit", self._lib.vf_jpeg_lut_submit, self._table_args(table, channels),
                                 jpegs, None, quality, subsamp, flags)

    def jpeg_lut_submit_addrs(self, addrs: np.ndarray, sizes: np.ndarray, table, channels: int, quality: int,
                              subsamp: int, flags: int = 0) -> int:
        """``jpeg_lut_submit`` from address / size arrays (the JPEGs in a worker's ring slots)."""
        return self._jpeg_submit("jpeg_lut_submit_addrs", self._lib.vf_jpeg_lut_submit,
                                 self._table_args(table, channels), addrs, sizes, quality, subsamp, flags)

    def jpeg_bench_lut(self, jpegs: Sequence, table, channels: int, quality: int, subsamp: int, flags: int = 0,
                       iters: int = 10):
        """``jpeg_bench_invert`` with the table in the colour stage."""
        return self._jpeg_bench(self._lib.vf_jpeg_bench_lut, self._table_args(table, channels), "color_lut", jpegs,
                                quality, subsamp, flags, iters)

    # -- JPEG with a convolution in place of the inversion (vf_jpeg_conv*); tickets are invert tickets ----
    def jpeg_conv(self, jpegs: Sequence, weights, shift: int, border: int, quality: int, subsamp: int,
                  flags: int = 0) -> list:
        """decode -> cv2.filter2D -> encode for every JPEG on the GPU; returns bytes."""
        if len(jpegs) == 0:
            return []
        ticket = self.jpeg_conv_submit(jpegs, weights, shift, border, quality, subsamp, flags)
        return [v.tobytes() for v in self.jpeg_invert_result(ticket)]

    def jpeg_conv_submit(self, jpegs: Sequence, weights, shift: int, border: int, quality: int, subsamp: int,
                         flags: int = 0) -> int:
        """``jpeg_invert_submit`` with the kernel; collect with the ``jpeg_invert_result*`` methods."""
        return self._jpeg_submit("jpeg_conv_submit", self._lib.vf_jpeg_conv_submit,
                                 self._weights_args(weights, shift, border), jpegs, None, quality, subsamp, flags)

    def jpeg_conv_submit_addrs(self, addrs: np.ndarray, sizes: np.ndarray, weights, shift: int, border: int,
                               quality: int, subsamp: int, flags: int = 0) -> int:
        """``jpeg_conv_submit`` from address / size arrays (the JPEGs in a worker's ring slots)."""
        return self._jpeg_submit("jpeg_conv_submit_addrs", self._lib.vf_jpeg_conv_submit,
                                 self._weights_args(weights, shift, border), addrs, sizes, quality, subsamp, flags)

    def jpeg_bench_conv(self, jpegs: Sequence, weights, shift: int, border: int, quality: int, subsamp: int,
                        flags: int = 0, iters: int = 10):
        """``jpeg_bench_invert`` with the convolution between the decode and the encode (its time is
        in the total, not in a stage: it runs between the colour and the fdct stage events)."""
        return self._jpeg_bench(self._lib.vf_jpeg_bench_conv, self._weights_args(weights, shift, border), "color",
                                jpegs, quality, subsamp, flags, iters)

    # -- JPEG with a rank filter in place of the inversion (vf_jpeg_rank*); tickets are invert tickets ----
    def jpeg_rank(self, jpegs: Sequence, op: int, element, border: int, quality: int, subsamp: int,
                  flags: int = 0) -> list:
        """decode -> cv2.erode / dilate / medianBlur -> encode for every JPEG on the GPU; returns bytes."""
        if len(jpegs) == 0:
            return []
        ticket = self.jpeg_rank_submit(jpegs, op, element, border, quality, subsamp, flags)
        return [v.tobytes() for v in self.jpeg_invert_result(ticket)]

    def jpeg_rank_submit(self, jpegs: Sequence, op: int, element, border: int, quality: int, subsamp: int,
                         flags: int = 0) -> int:
        """``jpeg_invert_submit`` with the rank filter; collect with the ``jpeg_invert_result*`` methods."""
        return self._jpeg_submit("jpeg_rank_submit", self._lib.vf_jpeg_rank_submit,
                                 self._element_args(op, element, border), jpegs, None, quality, subsamp, flags)

    def jpeg_rank_submit_addrs(self, addrs: np.ndarray, sizes: np.ndarray, op: int, element, border: int,
                               quality: int, subsamp: int, flags: int = 0) -> int:
        """``jpeg_rank_submit`` from address / size arrays (the JPEGs in a worker's ring slots)."""
        return self._jpeg_submit("jpeg_rank_submit_addrs", self._lib.vf_jpeg_rank_submit,
                                 self._element_args(op, element, border), addrs, sizes, quality, subsamp, flags)

    def jpeg_bench_rank(self, jpegs: Sequence, op: int, element, border: int, quality: int, subsamp: int,
                        flags: int = 0, iters: int = 10):
        """``jpeg_bench_invert`` with the rank filter between the decode and the encode (its time is
        in the total, not in a stage, as ``jpeg_bench_conv``'s)."""
        return self._jpeg_bench(self._lib.vf_jpeg_bench_rank, self._element_args(op, element, border), "color",
                                jpegs, quality, subsamp, flags, iters)

    # -- JPEG with a colour matrix in place of the inversion (vf_jpeg_mix*); tickets are invert tickets ----
    def _matrix_args(self, matrix, shift: int, rounding: int) -> tuple:
        return self._matrix(matrix).ctypes.data_as(_vp), shift, rounding

    def jpeg_mix(self, jpegs: Sequence, matrix, shift: int, rounding: int, quality: int, subsamp: int,
                 flags: int = 0) -> list:
        """decode -> cv2.transform -> encode for every JPEG on the GPU; returns bytes."""
        if len(jpegs) == 0:
            return []
        ticket = self.jpeg_mix_submit(jpegs, matrix, shift, rounding, quality, subsamp, flags)
        return [v.tobytes() for v in self.jpeg_invert_result(ticket)]

    def jpeg_mix_submit(self, jpegs: Sequence, matrix, shift: int, rounding: int, quality: int, subsamp: int,
                        flags: int = 0) -> int:
        """``jpeg_invert_submit`` with the matrix (copied by the library); collect with the
        ``jpeg_invert_result*`` methods."""
        return self._jpeg_submit("jpeg_mix_submit", self._lib.vf_jpeg_mix_submit,
                                 self._matrix_args(matrix, shift, rounding), jpegs, None, quality, subsamp, flags)

    def jpeg_mix_submit_addrs(self, addrs: np.ndarray, sizes: np.ndarray, matrix, shift: int, rounding: int,
                              quality: int, subsamp: int, flags: int = 0) -> int:
        """``jpeg_mix_submit`` from address / size arrays (the JPEGs in a worker's ring slots)."""
        return self._jpeg_submit("jpeg_mix_submit_addrs", self._lib.vf_jpeg_mix_submit,
                                 self._matrix_args(matrix, shift, rounding), addrs, sizes, quality, subsamp, flags)

    def jpeg_bench_mix(self, jpegs: Sequence, matrix, shift: int, rounding: int, quality: int, subsamp: int,
                       flags: int = 0, iters: int = 10):
        """``jpeg_bench_invert`` with the matrix between the decode and the encode (its time is in the
        total, not in a stage, as ``jpeg_bench_conv``'s)."""
        return self._jpeg_bench(self._lib.vf_jpeg_bench_mix, self._matrix_args(matrix, shift, rounding), "color",
                                jpegs, quality, subsamp, flags, iters)

    # -- JPEG with a separable filter in place of the inversion (vf_jpeg_sep*); tickets are invert tickets ----
    def _taps_args(self, kx, ky, shift: int, divisor: int, rounding: int, border: int) -> tuple:
        x, y = self._taps(kx), self._taps(ky)
        return x.ctypes.data_as(_vp), x.size, y.ctypes.data_as(_vp), y.size, shift, divisor, rounding, border

    def jpeg_sep(self, jpegs: Sequence, kx, ky, shift: int, divisor: int, rounding: int, border: int, quality: int,
                 subsamp: int, flags: int = 0) -> list:
        """decode -> cv2.sepFilter2D / cv2.blur -> encode for every JPEG on the GPU; returns bytes."""
        if len(jpegs) == 0:
            return []
        ticket = self.jpeg_sep_submit(jpegs, kx, ky, shift, divisor, rounding, border, quality, subsamp, flags)
        return [v.tobytes() for v in self.jpeg_invert_result(ticket)]

    def jpeg_sep_submit(self, jpegs: Sequence, kx, ky, shift: int, divisor: int, rounding: int, border: int,
                        quality: int, subsamp: int, flags: int = 0) -> int:
        """``jpeg_invert_submit`` with the taps (copied by the library); collect with the
        ``jpeg_invert_result*`` methods."""
        return self._jpeg_submit("jpeg_sep_submit", self._lib.vf_jpeg_sep_submit,
                                 self._taps_args(kx, ky, shift, divisor, rounding, border), jpegs, None, quality,
                                 subsamp, flags)

    def jpeg_sep_submit_addrs(self, addrs: np.ndarray, sizes: np.ndarray, kx, ky, shift: int, divisor: int,
                              rounding: int, border: int, quality: int, subsamp: int, flags: int = 0) -> int:
        """``jpeg_sep_submit`` from address / size arrays (the JPEGs in a worker's ring slots)."""
        return self._jpeg_submit("jpeg_sep_submit_addrs", self._lib.vf_jpeg_sep_submit,
                                 self._taps_args(kx, ky, shift, divisor, rounding, border), addrs, sizes, quality,
                                 subsamp, flags)

    def jpeg_bench_sep(self, jpegs: Sequence, kx, ky, shift: int, divisor: int, rounding: int, border: int,
                       quality: int, subsamp: int, flags: int = 0, iters: int = 10):
        """``jpeg_bench_invert`` with the separable filter between the decode and the encode (its time is in
        the total, not in a stage, as ``jpeg_bench_conv``'s)."""
        return self._jpeg_bench(self._lib.vf_jpeg_bench_sep, self._taps_args(kx, ky, shift, divisor, rounding, border),
                                "color", jpegs, quality, subsamp, flags, iters)

    # -- JPEG with the level filter in place of the inversion (vf_jpeg_level*); tickets are invert tickets ----
    def jpeg_level(self, jpegs: Sequence, rule: int, mask: int, link: int, clip_lo: int, clip_hi: int, quality: int,
                   subsamp: int, flags: int = 0) -> list:
        """decode -> cv2.equalizeHist / auto-levels -> encode for every JPEG on the GPU, each frame by its own
        histogram; returns bytes."""
        if len(jpegs) == 0:
            return []
        ticket = self.jpeg_level_submit(jpegs, rule, mask, link, clip_lo, clip_hi, quality, subsamp, flags)
        return [v.tobytes() for v in self.jpeg_invert_result(ticket)]

    def jpeg_level_submit(self, jpegs: Sequence, rule: int, mask: int, link: int, clip_lo: int, clip_hi: int,
                          quality: int, subsamp: int, flags: int = 0) -> int:
        """``jpeg_invert_submit`` with the level filter; collect with the ``jpeg_invert_result*`` methods."""
        return self._jpeg_submit("jpeg_level_submit", self._lib.vf_jpeg_level_submit,
                                 (rule, mask, link, clip_lo, clip_hi), jpegs, None, quality, subsamp, flags)

    def jpeg_level_submit_addrs(self, addrs: np.ndarray, sizes: np.ndarray, rule: int, mask: int, link: int,
                                clip_lo: int, clip_hi: int, quality: int, subsamp: int, flags: int = 0) -> int:
        """``jpeg_level_submit`` from address / size arrays (the JPEGs in a worker's ring slots)."""
        return self._jpeg_submit("jpeg_level_submit_addrs", self._lib.vf_jpeg_level_submit,
                                 (rule, mask, link, clip_lo, clip_hi), addrs, sizes, quality, subsamp, flags)

    def jpeg_bench_level(self, jpegs: Sequence, rule: int, mask: int, link: int, clip_lo: int, clip_hi: int,
                         quality: int, subsamp: int, flags: int = 0, iters: int = 10):
        """``jpeg_bench_invert`` with the level filter between the decode and the encode (its time is in the
        total, not in a stage, as ``jpeg_bench_conv``'s)."""
        return self._jpeg_bench(self._lib.vf_jpeg_bench_level, (rule, mask, link, clip_lo, clip_hi), "color", jpegs,
                                quality, subsamp, flags, iters)

    # -- JPEG with CLAHE in place of the inversion (vf_jpeg_clahe*); tickets are invert tickets --------------
    def jpeg_clahe(self, jpegs: Sequence, clip_q8: int, tiles_x: int, tiles_y: int, mask: int, quality: int,
                   subsamp: int, flags: int = 0) -> list:
        """decode -> CLAHE -> encode for every JPEG on the GPU; returns bytes."""
        if len(jpegs) == 0:
            return []
        ticket = self.jpeg_clahe_submit(jpegs, clip_q8, tiles_x, tiles_y, mask, quality, subsamp, flags)
        return [v.tobytes() for v in self.jpeg_invert_result(ticket)]

    def jpeg_clahe_submit(self, jpegs: Sequence, clip_q8: int, tiles_x: int, tiles_y: int, mask: int, quality: int,
                          subsamp: int, flags: int = 0) -> int:
        """``jpeg_invert_submit`` with CLAHE; collect with the ``jpeg_invert_result*`` methods."""
        return self._jpeg_submit("jpeg_clahe_submit", self._lib.vf_jpeg_clahe_submit, (clip_q8, tiles_x, tiles_y, mask),
                                 jpegs, None, quality, subsamp, flags)

    def jpeg_clahe_submit_addrs(self, addrs: np.ndarray, sizes: np.ndarray, clip_q8: int, tiles_x: int, tiles_y: int,
                                mask: int, quality: int, subsamp: int, flags: int = 0) -> int:
        """``jpeg_clahe_submit`` from address / size arrays (the JPEGs in a worker's ring slots)."""
        return self._jpeg_submit("jpeg_clahe_submit_addrs", self._lib.vf_jpeg_clahe_submit,
                                 (clip_q8, tiles_x, tiles_y, mask), addrs, sizes, quality, subsamp, flags)

    def jpeg_bench_clahe(self, jpegs: Sequence, clip_q8: int, tiles_x: int, tiles_y: int, mask: int, quality: int,
                         subsamp: int, flags: int = 0, iters: int = 10):
        """``jpeg_bench_invert`` with CLAHE between the decode and the encode (its time is in the total, not in a
        stage, as ``jpeg_bench_conv``'s)."""
        return self._jpeg_bench(self._lib.vf_jpeg_bench_clahe, (clip_q8, tiles_x, tiles_y, mask), "color", jpegs, quality,
                                subsamp, flags, iters)

    # -- JPEG with the affine warp in place of the inversion (vf_jpeg_warp*); tickets are invert tickets -----
    def jpeg_warp(self, jpegs: Sequence, m, mode: int, interp: int, border: int, value, quality: int, subsamp: int,
                  flags: int = 0) -> list:
        """decode -> warp -> encode for every JPEG on the GPU; returns bytes."""
        if len(jpegs) == 0:
            return []
        ticket = self.jpeg_warp_submit(jpegs, m, mode, interp, border, value, quality, subsamp, flags)
        return [v.tobytes() for v in self.jpeg_invert_result(ticket)]

    def jpeg_warp_submit(self, jpegs: Sequence, m, mode: int, interp: int, border: int, value, quality: int,
                         subsamp: int, flags: int = 0) -> int:
        """``jpeg_invert_submit`` with the warp; collect with the ``jpeg_invert_result*`` methods."""
        return self._jpeg_submit("jpeg_warp_submit", self._lib.vf_jpeg_warp_submit,
                                 self._warp_args(m, mode, interp, border, value), jpegs, None, quality, subsamp, flags)

    def jpeg_warp_submit_addrs(self, addrs: np.ndarray, sizes: np.ndarray, m, mode: int, interp: int, border: int, value,
                               quality: int, subsamp: int, flags: int = 0) -> int:
        """``jpeg_warp_submit`` from address / size arrays (the JPEGs in a worker's ring slots)."""
        return self._jpeg_submit("jpeg_warp_submit_addrs", self._lib.vf_jpeg_warp_submit,
                                 self._warp_args(m, mode, interp, border, value), addrs, sizes, quality, subsamp, flags)

    # -- JPEG with the resize in place of the inversion (vf_jpeg_resize*); tickets are invert tickets ---------
    @staticmethod
    def _resize_args(dw, dh, fx, fy, interp) -> tuple:
        """``filters.Resize.args`` as the C arguments."""
        return int(dw), int(dh), float(fx), float(fy), int(interp)

    def jpeg_resize(self, jpegs: Sequence, dw: int, dh: int, fx: float, fy: float, interp: int, quality: int, subsamp: int,
                    flags: int = 0) -> list:
        """decode -> resize -> encode for every JPEG on the GPU; returns bytes, each of its result's size."""
        if len(jpegs) == 0:
            return []
        ticket = self.jpeg_resize_submit(jpegs, dw, dh, fx, fy, interp, quality, subsamp, flags)
        return [v.tobytes() for v in self.jpeg_invert_result(ticket)]

    def jpeg_resize_submit(self, jpegs: Sequence, dw: int, dh: int, fx: float, fy: float, interp: int, quality: int,
                           subsamp: int, flags: int = 0) -> int:
        """``jpeg_invert_submit`` with the resize; collect with the ``jpeg_invert_result*`` methods."""
        return self._jpeg_submit("jpeg_resize_submit", self._lib.vf_jpeg_resize_submit,
                                 self._resize_args(dw, dh, fx, fy, interp), jpegs, None, quality, subsamp, flags)

    def jpeg_resize_submit_addrs(self, addrs: np.ndarray, sizes: np.ndarray, dw: int, dh: int, fx: float, fy: float,
                                 interp: int, quality: int, subsamp: int, flags: int = 0) -> int:
        """``jpeg_resize_submit`` from address / size arrays (the JPEGs in a worker's ring slots)."""
        return self._jpeg_submit("jpeg_resize_submit_addrs", self._lib.vf_jpeg_resize_submit,
                                 self._resize_args(dw, dh, fx, fy, interp), addrs, sizes, quality, subsamp, flags)

    def jpeg_bench_resize(self, jpegs: Sequence, dw: int, dh: int, fx: float, fy: float, interp: int, quality: int,
                          subsamp: int, flags: int = 0, iters: int = 10):
        """``jpeg_bench_invert`` with the resize between the decode and the encode."""
        return self._jpeg_bench(self._lib.vf_jpeg_bench_resize, self._resize_args(dw, dh, fx, fy, interp), "color",
                                jpegs, quality, subsamp, flags, iters)

    def jpeg_bench_warp(self, jpegs: Sequence, m, mode: int, interp: int, border: int, value, quality: int,
                        subsamp: int, flags: int = 0, iters: int = 10):
        """``jpeg_bench_invert`` with the warp between the decode and the encode (its time is in the total, not in a
        stage, as ``jpeg_bench_conv``'s)."""
        return self._jpeg_bench(self._lib.vf_jpeg_bench_warp, self._warp_args(m, mode, interp, border, value), "color",
                                jpegs, quality, subsamp, flags, iters)

    # -- JPEG with a filter chain in place of the inversion (vf_jpeg_chain*); tickets are invert tickets ----
    def jpeg_chain(self, jpegs: Sequence, steps: Sequence, quality: int, subsamp: int, flags: int = 0) -> list:
        """decode -> the program's steps -> encode for every JPEG on the GPU; returns bytes.  ``steps``
        as for ``chain_frames_host`` (``filters.Chain.args[0]``)."""
        if len(jpegs) == 0:
            return []
        ticket = self.jpeg_chain_submit(jpegs, steps, quality, subsamp, flags)
        return [v.tobytes() for v in self.jpeg_invert_result(ticket)]

    def jpeg_chain_submit(self, jpegs: Sequence, steps: Sequence, quality: int, subsamp: int, flags: int = 0) -> int:
        """``jpeg_invert_submit`` with the program (copied by the library: the caller may change its
        arrays at once); collect with the ``jpeg_invert_result*`` methods."""
        arr, keep = self._steps(steps)
        t = self._jpeg_submit("jpeg_chain_submit", self._lib.vf_jpeg_chain_submit, (arr, len(steps)), jpegs, None,
                              quality, subsamp, flags)
        del keep
        return t

    def jpeg_chain_submit_addrs(self, addrs: np.ndarray, sizes: np.ndarray, steps: Sequence, quality: int,
                                subsamp: int, flags: int = 0) -> int:
        """``jpeg_chain_submit`` from address / size arrays (the JPEGs in a worker's ring slots)."""
        arr, keep = self._steps(steps)
        t = self._jpeg_submit("jpeg_chain_submit_addrs", self._lib.vf_jpeg_chain_submit, (arr, len(steps)), addrs,
                              sizes, quality, subsamp, flags)
        del keep
        return t

    def jpeg_bench_chain(self, jpegs: Sequence, steps: Sequence, quality: int, subsamp: int, flags: int = 0,
                         iters: int = 10):
        """``jpeg_bench_invert`` with the program between the decode and the encode (its time is in the
        total, not in a stage, as ``jpeg_bench_conv``'s)."""
        arr, keep = self._steps(steps)
        out = self._jpeg_bench(self._lib.vf_jpeg_bench_chain, (arr, len(steps)), "color", jpegs, quality, subsamp,
                               flags, iters)
        del keep
        return out


def jpeg_header(jpeg) -> tuple:
    """(width, height, TJSAMP_*, TJCS_*) of a JPEG; host-only (vf_jpeg_header)."""
    lib = load_library()
    a = jpeg if isinstance(jpeg, np.ndarray) else np.frombuffer(jpeg, dtype=np.uint8)
    w, h, ss, cs = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    st = lib.vf_jpeg_header(a.ctypes.data, a.nbytes, ctypes.byref(w), ctypes.byref(h), ctypes.byref(ss),
                            ctypes.byref(cs))
    if st != VF_OK:
        raise VFilterError(lib.vf_last_error(None).decode(), st)
    return w.value, h.value, ss.value, cs.value


_default_ctx: Optional[Context] = None


def default_device() -> int:
    """GPU of this worker process: VF_DEVICE, else LOCAL_RANK, else 0.

    One process owns one GPU; a launcher that sets HIP_VISIBLE_DEVICES per
    worker leaves the visible ordinal at 0.
    """
    for var in ("VF_DEVICE", "LOCAL_RANK"):
        v = os.environ.get(var)
        if v not in (None, ""):
            return int(v)
    return 0


_deferred_lock = threading.Lock()
_deferred: list = []  # closed contexts whose last pinned result array is gone


def _defer_destroy(ctx: "Context") -> None:
    with _deferred_lock:
        _deferred.append(ctx)


def reap_closed_contexts() -> int:
    """Destroy the library contexts of closed ``Context`` objects whose pinned result arrays are
    all gone; returns how many.  Runs at each ``Context()`` and at exit."""
    with _deferred_lock:
        todo = _deferred[:]
        _deferred.clear()
    for c in todo:
        c.close()  # its arena's free blocks back to the library, then vf_destroy
    return len(todo)


atexit.register(reap_closed_contexts)


def get_context() -> Context:
    """Process-wide default context (created on first use)."""
    global _default_ctx
    if _default_ctx is None:
        _default_ctx = Context(default_device())
    return _default_ctx
