"""Drop-in for ``CViT-main/ResKan/kan_resnet.py``.

The reference trainer imports its model with ``sys.path.insert(1, 'model');
from kan_resnet import resnet34`` (ResKan_train.py).  Pointing that path at
this directory swaps in the gfx950 HIP implementation with the same
constructor, state_dict and forward contract.
"""
import os
import sys

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if _ROOT not in sys.path:
    sys.path.insert(0, _ROOT)

from fac_fake_amd.reskan import ResNet, resnet34  # noqa: E402,F401

__all__ = ["ResNet", "resnet34"]
