"""Drop-in for ``CViT-main/model/other/cvit_GGCA_ADD_WTConv.py`` (WTConv2d(C) -> BatchNorm -> ReLU in place of nine 3x3 convs of features, x + GGCA(x) after the stem).

The reference's users copy this file next to ``cvit.py`` and edit the import
line; from here or from there, ``from cvit_GGCA_ADD_WTConv import CViT`` gives the gfx950
HIP implementation with the same constructor, state_dict and forward contract
(fac_fake_amd/wtconv.py).
"""
import os
import sys

_DIR = os.path.dirname(os.path.abspath(__file__))
for _up in (1, 2):      # model/other/<this file> here, model/<this file> when copied next to cvit.py
    _ROOT = os.path.normpath(os.path.join(_DIR, *[".."] * _up))
    if os.path.isdir(os.path.join(_ROOT, "fac_fake_amd")) and _ROOT not in sys.path:
        sys.path.insert(0, _ROOT)

from fac_fake_amd.wtconv import CViT  # noqa: E402

__all__ = ["CViT"]
