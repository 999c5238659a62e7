"""Dump the raw bits of the fourteen CViT variants' logits, for comparing two
revisions of the Python side bit for bit (the goldens are tolerance-based).

  python tools/dump_family_logits.py --out A.npz           # on each revision, same machine
  python tools/dump_family_logits.py --compare A.npz B.npz

For each class (RepBn8, weights.VARIANTS, cvit_GGCA_ADD_DConv,
weights.OTHER_VARIANTS) and both dtypes: the seed-0 synthetic weights,
``forward_u8`` on ``make_crops(4, seed=31)`` with slots 0..3 and ``forward`` on
the normalised fp32 form of the same crops; the logits as uint32.  For RepBn8
also ``gradcam_features``' two maps as int16.  The kernels have a fixed
summation order and no value-carrying atomics, so two revisions that launch
the same kernels with the same arguments give equal arrays.  It only uses
entry points both sides of such a comparison have (``cvit_prediction``'s
loader), and needs a GPU.
"""
from __future__ import annotations

import argparse
import sys
from pathlib import Path

sys.dont_write_bytecode = True
REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))

import numpy as np  # noqa: E402

CROP_SEED, N_CROPS = 31, 4
REPBN8, DCONV = "cvit_GGCA_ADD_DEConv_RepBn8", "cvit_GGCA_ADD_DConv"


def dump(out: str) -> None:
    import torch

    import cvit_prediction as P
    from fac_fake_amd.weights import OTHER_NAMES, VARIANT_NAMES, make_crops
    from oracle.cvit_torch import normalize_u8
    if not torch.cuda.is_available():
        raise SystemExit("dump_family_logits.py needs a GPU")
    crops = make_crops(N_CROPS, seed=CROP_SEED)
    u8 = torch.from_numpy(crops).cuda()
    img = normalize_u8(crops).cuda()
    slots = torch.arange(N_CROPS, dtype=torch.int32, device="cuda")
    arrays = {}
    for name in (REPBN8, *VARIANT_NAMES, DCONV, *OTHER_NAMES):
        sd = {k: torch.from_numpy(np.asarray(v)) for k, v in P._synthetic_state_dict(name).items()}
        for dt in ("fp16", "bf16"):
            m = P.model_class(name)(dtype=dt)
            m.load_state_dict(sd)
            m.to("cuda")
            with torch.no_grad():
                arrays[f"{name}/{dt}/forward_u8"] = m.forward_u8(u8, pos_index=slots).cpu().numpy().view(np.uint32)
                arrays[f"{name}/{dt}/forward"] = m(img, pos_index=slots).cpu().numpy().view(np.uint32)
                if name == REPBN8:
                    a, feat = m.gradcam_features(u8, True)
                    arrays[f"{name}/{dt}/gradcam_a"] = a.view(torch.int16).cpu().numpy()
                    arrays[f"{name}/{dt}/gradcam_feat"] = feat.view(torch.int16).cpu().numpy()
            torch.cuda.synchronize()
            m._release()
            print(f"{name} {dt}: {arrays[f'{name}/{dt}/forward_u8'].reshape(-1)[:2]}", flush=True)
    np.savez(out, **arrays)
    print(f"wrote {out}: {len(arrays)} arrays")


def compare(a: str, b: str) -> int:
    x, y = np.load(a), np.load(b)
    bad = sorted(set(x.files) ^ set(y.files))
    lines = [f"{a} vs {b}: {len(x.files)} and {len(y.files)} arrays"]
    lines += [f"  only on one side: {k}" for k in bad]
    for k in sorted(set(x.files) & set(y.files)):
        same = x[k].shape == y[k].shape and x[k].dtype == y[k].dtype and np.array_equal(x[k], y[k])
        lines.append(f"  {'equal   ' if same else 'DIFFERS '} {k} {x[k].dtype}{list(x[k].shape)}")
        if not same:
            bad.append(k)
    lines.append("every array is bit-identical" if not bad else f"{len(bad)} arrays differ or are missing")
    print("\n".join(lines))
    return 1 if bad else 0


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", help="write this revision's arrays to an .npz")
    ap.add_argument("--compare", nargs=2, metavar=("A", "B"), help="compare two such files")
    args = ap.parse_args(argv)
    if args.compare:
        raise SystemExit(compare(*args.compare))
    if not args.out:
        ap.error("--out or --compare")
    dump(args.out)


if __name__ == "__main__":
    main()
