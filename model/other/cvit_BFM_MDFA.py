"""Drop-in for ``CViT-main/model/other/cvit_BFM_MDFA.py`` (x = BFM(256)(x, x) after features1, x = MDFA(512, 512)(x) after the stem; its ggca is never called).

The reference's users copy this file next to ``cvit.py`` and edit the import
line; from here or from there, ``from cvit_BFM_MDFA import CViT`` gives the gfx950
HIP implementation with the same constructor, state_dict and forward contract
(fac_fake_amd/mdfa.py).
"""
import os
import sys

_DIR = os.path.dirname(os.path.abspath(__file__))
for _up in (1, 2):      # model/other/<this file> here, model/<this file> when copied next to cvit.py
    _ROOT = os.path.normpath(os.path.join(_DIR, *[".."] * _up))
    if os.path.isdir(os.path.join(_ROOT, "fac_fake_amd")) and _ROOT not in sys.path:
        sys.path.insert(0, _ROOT)

from fac_fake_amd.mdfa import mdfa_class  # noqa: E402

CViT = mdfa_class("cvit_BFM_MDFA")

__all__ = ["CViT"]
