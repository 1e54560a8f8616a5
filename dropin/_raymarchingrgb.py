"""Import-compatible stand-in for the pybind module `_raymarchingrgb` (/root/reference/core/nerf/raymarching/rgb/src/bindings.cpp), found
by the reference's rgb/raymarching.py:14-27 through PYTHONPATH.  Body: dropin/_raymarching_backend.py (3 colour channels, `binarize`)."""
import os as _os
import sys as _sys

_sys.path.insert(0, _os.path.dirname(_os.path.abspath(__file__)))
try:
    import _raymarching_backend as _b
finally:
    _sys.path.pop(0)

globals().update(_b.functions(3, binarize=True))
__all__ = list(_b.NAMES)
