"""Drop-in for ``CViT-main/model/other/cvit_GGCA_ADD_ScConv.py`` (ScConv(C) -> BatchNorm -> ReLU in place of four 3x3 convs of features1, x + GGCA(x) after the stem).

The reference's users copy this file next to ``cvit.py`` and edit the import
line; from here or from there, ``from cvit_GGCA_ADD_ScConv import CViT`` gives the gfx950
HIP implementation with the same constructor, state_dict and forward contract
(fac_fake_amd/scconv.py).
"""
import os
import sys

_DIR = os.path.dirname(os.path.abspath(__file__))
for _up in (1, 2):      # model/other/<this file> here, model/<this file> when copied next to cvit.py
    _ROOT = os.path.normpath(os.path.join(_DIR, *[".."] * _up))
    if os.path.isdir(os.path.join(_ROOT, "fac_fake_amd")) and _ROOT not in sys.path:
        sys.path.insert(0, _ROOT)

from fac_fake_amd.scconv import scconv_class  # noqa: E402

CViT = scconv_class("cvit_GGCA_ADD_ScConv")

__all__ = ["CViT"]
