"""Measure fac_fake_amd.weights.MSCA_S3D_BN_CAL: per BatchNorm of msca_S3D, the
mean and variance of its input over the fixture clips.

Runs the project's own fp32 restatement (tests/msca_s3d_ref.py) on the 4
content-varied 16 x 112 x 112 fixture clips, layer by layer: before a BatchNorm
is applied, the mean and variance of its input are taken over everything, its
running statistics are drawn around them (weights.msca_s3d_running, what
make_msca_s3d_state_dict does with the table), and only then does the forward
go on, so every later layer is measured behind calibrated ones.  Prints the
table to paste into weights.py; CPU only, about a second.

    python tools/calibrate_msca_s3d.py
"""
from __future__ import annotations

import sys
from pathlib import Path

sys.dont_write_bytecode = True
REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(REPO / "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import msca_s3d_ref as R  # noqa: E402
from fac_fake_amd.weights import (make_msca_s3d_state_dict, msca_s3d_bn_names, msca_s3d_running,  # noqa: E402
                                  s3d_clips_varied)

CLIP_SEED, N_CLIPS = 43, 4


def calibrate(srm: bool, seed: int = 0):
    sd = R.cast_sd(make_msca_s3d_state_dict(seed, 1, srm, cal={}), torch.float32)
    x = torch.from_numpy(s3d_clips_varied(N_CLIPS, 16, 112, CLIP_SEED))
    cal = {}

    def hook(p, t):
        m, v = float(t.double().mean()), float(t.double().var(unbiased=False))
        m, v = float(np.float32(m)), float(np.float32(v))
        cal[p] = (m, v)
        for leaf in ("running_mean", "running_var"):
            sd[f"{p}.{leaf}"] = torch.from_numpy(msca_s3d_running(f"{p}.{leaf}", t.shape[1], seed, m, v))

    R.forward(sd, x, srm, bn_hook=hook)
    names = msca_s3d_bn_names(srm)
    assert set(cal) == set(names) and len(names) == 122
    return [cal[n] for n in names]


if __name__ == "__main__":
    torch.set_num_threads(16)
    print("MSCA_S3D_BN_CAL: dict = {")
    for srm in (False, True):
        rows = calibrate(srm)
        print(f"    {srm}: [")
        for i in range(0, len(rows), 4):
            print("        " + " ".join(f"({m:.6g}, {v:.6g})," for m, v in rows[i:i + 4]))
        print("    ],")
    print("}")
