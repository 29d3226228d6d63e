"""vfilter — MI355X-native backend for the per-frame filter of
kylemcdonald/distributed-video-filter (inverter.py inside worker.py, fanned out by
distributor.py).

  filters      ``bitwise_not`` (the ``cv2.bitwise_not`` drop-in, inverter.py:41) and batch forms;
               ``lut`` (the ``cv2.LUT`` drop-in: any other per-pixel filter) and ``lut_frames``
               ``filter2d`` (the ``cv2.filter2D`` drop-in: blur, sharpen, Sobel, ...) and
               ``filter2d_frames``
  tables       builders of the usual 256-entry tables (gamma, levels, threshold, posterize, ...)
               ``erode``, ``dilate``, ``median_blur`` (the ``cv2.erode`` / ``cv2.dilate`` /
               ``cv2.medianBlur`` drop-ins) and ``rank_frames``
               ``Chain`` / ``Combine`` / ``Morph`` (a program of the filters above in one GPU pass),
               ``chain``, ``chain_frames`` and ``morphology_ex`` (the ``cv2.morphologyEx`` drop-in)
               ``transform`` (the ``cv2.transform`` drop-in: a 3 x 3 colour matrix plus offset per
               pixel), ``Mix`` and ``transform_frames``
               ``sep_filter2d``, ``blur`` and ``box_filter`` (the ``cv2.sepFilter2D``, ``cv2.blur`` and
               ``cv2.boxFilter`` drop-ins: up to 31 taps an axis, the mean by an exact division),
               ``Separable`` and ``sep_frames``
               ``equalize_hist`` (the ``cv2.equalizeHist`` drop-in), ``auto_levels``, ``calc_hist`` (the
               histogram, counted on the GPU), ``Level``, ``level_frames`` and ``calc_hist_frames``
               ``clahe`` and ``create_clahe`` (the ``cv2.createCLAHE`` drop-in), ``Clahe`` and ``clahe_frames``
               ``warp_affine``, ``flip`` and ``rotate`` (the ``cv2.warpAffine``, ``cv2.flip`` and ``cv2.rotate(ROTATE_180)``
               drop-ins for frames that keep their size), ``Warp`` and ``warp_frames``
               ``resize`` (the ``cv2.resize`` drop-in: nearest, linear, area), ``Resize`` and ``resize_frames``
  warps        builders of the usual affine maps (rotation, translation, zoom)
  colors       builders of the usual colour matrices (gray, swap_rb, sepia, saturation, gain, ...)
  kernels      builders of the usual convolution kernels (gaussian3/5/7, sharpen, sobel_x, ...)
  elements     builders of the usual structuring elements (rect, cross)
  _lib         ctypes binding to libvfilter_hip.so (include/vfilter.h)

The worker loop, the inverter plugin and the distributor live in ``worker``,
``inverter`` and ``distributor`` (imported on demand; they need no GPU to import).
"""
from . import colors, elements, kernels, tables, warps  # noqa: F401
from ._lib import (ABI_VERSION, Context, VFilterError, device_count, get_context,  # noqa: F401
                   library_path, load_library)
from .filters import (Chain, Combine, Mix, Morph, Rank, as_element, as_kernel, as_matrix, as_table,  # noqa: F401
                      bitwise_not, chain,
                      chain_frames, dilate, erode, filter2d, filter2d_frames, invert, invert_batch, invert_bytes,
                      invert_frames, lut, lut_frames, median_blur, morphology_ex, rank_frames, transform,
                      transform_frames)
from .filters import Separable, as_taps, blur, box_filter, sep_filter2d, sep_frames  # noqa: F401
from .filters import Level, auto_levels, calc_hist, calc_hist_frames, equalize_hist, level_frames  # noqa: F401
from .filters import Clahe, clahe, clahe_frames, create_clahe  # noqa: F401
from .filters import Warp, flip, rotate, warp_affine, warp_frames  # noqa: F401
from .filters import Resize, resize, resize_frames  # noqa: F401

__all__ = [
    "ABI_VERSION", "Context", "VFilterError", "device_count", "get_context", "library_path",
    "load_library", "bitwise_not", "invert", "invert_batch", "invert_bytes", "invert_frames",
    "as_table", "lut", "lut_frames", "as_kernel", "filter2d", "filter2d_frames", "kernels", "tables",
    "Rank", "as_element", "erode", "dilate", "median_blur", "rank_frames", "elements",
    "Chain", "Combine", "Morph", "chain", "chain_frames", "morphology_ex",
    "Mix", "as_matrix", "transform", "transform_frames", "colors",
    "Separable", "as_taps", "sep_filter2d", "blur", "box_filter", "sep_frames",
    "Level", "equalize_hist", "auto_levels", "calc_hist", "calc_hist_frames", "level_frames",
    "Clahe", "clahe", "create_clahe", "clahe_frames",
    "Warp", "warp_affine", "flip", "rotate", "warp_frames", "warps",
    "Resize", "resize", "resize_frames",
]
