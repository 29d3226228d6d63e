"""Builders of the usual affine maps, as the 2 x 3 float64 forward matrices ``cv2.warpAffine`` and
``vfilter.warp_affine`` / ``vfilter.Warp`` take."""
import math

import numpy as np


def rotation(center, angle: float, scale: float = 1.0) -> np.ndarray:
    """``cv2.getRotationMatrix2D(center, angle, scale)``: ``angle`` in degrees, positive counter-clockwise (the
    origin is the top-left corner), about ``center = (x, y)``."""
    cx, cy = float(center[0]), float(center[1])
    rad = float(angle) * math.pi / 180.0
    a, b = float(scale) * math.cos(rad), float(scale) * math.sin(rad)
    return np.array([[a, b, (1 - a) * cx - b * cy], [-b, a, b * cx + (1 - a) * cy]], np.float64)


def translation(dx: float, dy: float) -> np.ndarray:
    """The content moves ``dx`` pixels to the right and ``dy`` down."""
    return np.array([[1.0, 0.0, float(dx)], [0.0, 1.0, float(dy)]], np.float64)


def zoom(factor: float, center) -> np.ndarray:
    """A digital zoom by ``factor`` that keeps ``center = (x, y)`` in place: ``rotation(center, 0, factor)``."""
    return rotation(center, 0.0, factor)
