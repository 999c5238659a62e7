"""Drop-in for ``CViT-main/figure/utils.py``'s ``GradCAM``.

With the reference's ``sys.path.insert(1, 'figure')`` pointed at this
directory, ``from utils import GradCAM`` gives the gfx950 HIP implementation
with the same constructor, context-manager use and call contract
(fac_fake_amd/gradcam.py).  ``show_cam_on_image`` and ``center_crop_img`` are
not provided (they need cv2's colormap table).
"""
import os
import sys

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if _ROOT not in sys.path:
    sys.path.insert(0, _ROOT)

from fac_fake_amd.gradcam import GradCAM  # noqa: E402,F401

__all__ = ["GradCAM"]
