"""Structuring elements for ``vfilter.erode`` / ``vfilter.dilate``: what
``cv2.getStructuringElement`` returns for ``MORPH_RECT`` and ``MORPH_CROSS`` with the anchor at the
centre, as uint8 0/1 arrays of ``h`` rows and ``w`` columns.  Sides are odd and at most 7.

``cv2.MORPH_ELLIPSE`` is not here: its rasterisation differs between OpenCV versions.
"""
from __future__ import annotations

from typing import Optional

import numpy as np


def _sides(w, h: Optional[int]) -> tuple:
    h = w if h is None else h
    for v in (w, h):
        if int(v) != v or not 1 <= v <= 7 or int(v) % 2 == 0:
            raise ValueError(f"a {w} x {h} element; sides must be odd and at most 7")
    return int(w), int(h)


def rect(w: int, h: Optional[int] = None) -> np.ndarray:
    """``cv2.getStructuringElement(cv2.MORPH_RECT, (w, h))``: all ones."""
    w, h = _sides(w, h)
    return np.ones((h, w), np.uint8)


def cross(w: int, h: Optional[int] = None) -> np.ndarray:
    """``cv2.getStructuringElement(cv2.MORPH_CROSS, (w, h))``: the centre row and the centre column."""
    w, h = _sides(w, h)
    e = np.zeros((h, w), np.uint8)
    e[h // 2, :] = 1
    e[:, w // 2] = 1
    return e
