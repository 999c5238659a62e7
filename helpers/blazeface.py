"""Drop-in for ``CViT-main/helpers/blazeface.py``.

The reference imports its detector with ``from helpers.blazeface import
BlazeFace`` (or ``sys.path.insert(1, 'helpers'); from blazeface import
BlazeFace``).  Pointing that path at this directory swaps in the gfx950 HIP
implementation with the same attributes, state_dict and prediction methods.
"""
import os
import sys

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if _ROOT not in sys.path:
    sys.path.insert(0, _ROOT)

from fac_fake_amd.blazeface import BlazeFace  # noqa: E402,F401

__all__ = ["BlazeFace"]
