"""Generate the CA_S3D_v3 fixtures under tests/golden/ from the REFERENCE itself.

Runs only where the reference tree is (it does not exist on the GPU box).  It
imports ``sx_exp_deepfakedetect-master/S3D/CA_S3D.py`` (plain torch + numpy),
loads the repo's deterministic synthetic weights
(fac_fake_amd.weights.make_ca_s3d_state_dict, seed 0, num_class 1) and records
the reference's outputs.  Data only:

  ca_s3d_keys.json    the reference state_dict's keys and shapes (SRM_net 'no'
                      and 'yes'), in order
  ca_s3d_golden_blocks.npz (SRM_net 'no'), ca_s3d_golden_blocks_srm.npz ('yes')
                      8 content-varied clips of 16 x 112 x 112
                      (s3d_clips_varied, seed 41) through CA_S3D_v3(1, 'no')
                      and (1, 'yes'): logits, the per-channel mean over
                      (T, H, W) of every base[i] output, the 16-bit rounding
                      envelope of each (tests/ca_s3d_ref.py's emulation of the
                      HIP path's rounding points vs the reference) and of the
                      probabilities and logits; and, per context block, the margins that
                      show the synthetic context weights matter (below)
  ca_s3d_golden_20x224.npz
                      2 clips at the harness shape (20 x 224 x 224, seed 37):
                      logits, probability and logit envelopes

For every context block the generator asserts, and records as
``ctx_{srm}_*`` (one entry per block, in base order):

  term_rms / in_rms   rms of the term over rms of the block's input, in [0.5, 2]
  ident_shift         how far replacing the block by the identity moves that
                      layer's channel means (max |.|, relative to the rms of
                      the reference means: the GPU test's measure), at least
                      10x the GPU test's gate 2 env + 1e-4
  clip_diff           the largest per-channel difference of term between two
                      clips, at least 10x that gate times the input rms

    python tools/make_golden_ca_s3d.py [--harness-shape]
"""
from __future__ import annotations

import json
import sys
from pathlib import Path

sys.dont_write_bytecode = True
REPO = Path(__file__).resolve().parents[1]
REF = Path("/root/reference/sx_exp_deepfakedetect-master/S3D")
OUT = REPO / "tests" / "golden"
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(REPO / "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from fac_fake_amd.weights import ca_s3d_base, make_ca_s3d_state_dict, s3d_clips_varied  # noqa: E402


def _rel(a, b):
    """max |a - b| over everything, relative to the rms of b."""
    return float(np.abs(a - b).max() / (np.sqrt((b.astype(np.float64) ** 2).mean()) + 1e-30))


def _rms(t):
    return float(np.sqrt((np.asarray(t, dtype=np.float64) ** 2).mean()))


def _model(CA, srm):
    m = CA(1, srm).eval()
    sd = make_ca_s3d_state_dict(0, 1, srm == "yes")
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    return m, sd


def _envelopes(R, sd, x, srm, lg, out, means=None):
    p_ref = 1 / (1 + np.exp(-lg.astype(np.float64)))
    for dt in ("fp16", "bf16"):
        if means is not None:
            et = []
            R.features_emulated(sd, x, srm == "yes", dt, et)
            out[f"env_{srm}_{dt}"] = np.array([_rel(t.double().mean(dim=(2, 3, 4)).numpy(), mu)
                                              for t, mu in zip(et, means)])
        le = R.forward_emulated(sd, x, srm == "yes", dt).double().numpy()
        pe = 1 / (1 + np.exp(-le))
        out[f"env_prob_{srm}_{dt}"] = np.float64(np.abs(pe - p_ref).max())
        out[f"env_logit_{srm}_{dt}"] = np.float64(np.abs(le - lg.astype(np.float64)).max())
    return p_ref


def blocks(CA):
    import ca_s3d_ref as R  # the restatement + rounding-point emulation, for envelopes and margins only
    seed, n = 41, 8
    x = torch.from_numpy(s3d_clips_varied(n, 16, 112, seed))
    out = {"clip_seed": np.int64(seed), "n_clips": np.int64(n)}
    keys, bad = {}, []
    for srm in ("no", "yes"):
        m, sd = _model(CA, srm)
        keys[srm] = [[k, list(v.shape)] for k, v in m.state_dict().items()]
        taps = []
        hooks = [m.base[i].register_forward_hook(lambda mod, i_, o: taps.append(o.detach().clone()))
                 for i in range(len(m.base))]
        with torch.no_grad():
            lg = m(x).numpy()
        for h in hooks:
            h.remove()
        assert len(taps) == 22
        means = [t.double().mean(dim=(2, 3, 4)).numpy() for t in taps]
        out[f"logits_{srm}"] = lg
        for i, mu in enumerate(means):
            out[f"mean_{srm}_{i}"] = mu.astype(np.float32)
        p_ref = _envelopes(R, sd, x, srm, lg, out, means)
        # the context blocks' margins
        ctx_idx = [i for i, L in enumerate(ca_s3d_base(srm == "yes")) if L[0] == "ctx"]
        rec = {k: [] for k in ("term_rms", "in_rms", "ident_shift", "clip_diff", "gate")}
        for i in ctx_idx:
            xin = taps[i - 1]
            term = (taps[i] - xin)[:, :, 0, 0, 0].double().numpy()            # [n, C]: the broadcast term itself
            gate = 2 * float(out[f"env_{srm}_fp16"][i]) + 1e-4, 2 * float(out[f"env_{srm}_bf16"][i]) + 1e-4
            ident = _rel(xin.double().mean(dim=(2, 3, 4)).numpy(), means[i])  # base[i] replaced by the identity
            diff = float(np.abs(term[:, None, :] - term[None, :, :]).max())
            rec["term_rms"].append(_rms(term))
            rec["in_rms"].append(_rms(xin))
            rec["ident_shift"].append(ident)
            rec["clip_diff"].append(diff)
            rec["gate"].append(max(gate))
            print(f"  ctx base.{i}: term rms {_rms(term):.4f} input rms {_rms(xin):.4f} identity shift {ident:.3f} "
                  f"clip diff {diff:.4f} gate {max(gate):.2e}")
            if not 0.5 * _rms(xin) <= _rms(term) <= 2 * _rms(xin):
                bad.append((srm, i, "term rms outside 0.5x..2x the input rms"))
            if not ident >= 10 * max(gate):
                bad.append((srm, i, "the identity would pass the GPU gate"))
            if not diff >= 10 * max(gate) * _rms(xin):
                bad.append((srm, i, "term hardly differs between clips"))
        for k, v in rec.items():
            out[f"ctx_{srm}_{k}"] = np.array(v, dtype=np.float64)
        out[f"ctx_{srm}_index"] = np.array(ctx_idx, dtype=np.int64)
        print(srm, "probs", np.round(p_ref.ravel(), 4), "env fp16", np.round(out[f"env_{srm}_fp16"], 4),
              "bf16", np.round(out[f"env_{srm}_bf16"], 4), out[f"env_prob_{srm}_fp16"], out[f"env_prob_{srm}_bf16"],
              "logits", np.round(lg.ravel(), 3), "env_logit", out[f"env_logit_{srm}_fp16"], out[f"env_logit_{srm}_bf16"])
    # a weight range that cannot meet these is changed in weights.py, never the conditions
    assert not bad, bad
    (OUT / "ca_s3d_keys.json").write_text(json.dumps(keys))
    # one file per SRM setting (each within the size of the earlier fixtures); the clip keys go with 'no'
    yes = {k: v for k, v in out.items() if "_yes" in k}
    np.savez_compressed(OUT / "ca_s3d_golden_blocks.npz", **{k: v for k, v in out.items() if k not in yes})
    np.savez_compressed(OUT / "ca_s3d_golden_blocks_srm.npz", **yes)


def harness_shape(CA):
    """2 raw clips of 20 x 224 x 224 (S3D-test.py:130-190; s3d_clips_varied, seed 37)."""
    import ca_s3d_ref as R
    x = torch.from_numpy(s3d_clips_varied(2, 20, 224, seed=37))
    out = {"clip_seed": np.int64(37), "frames": np.int64(20), "size": np.int64(224)}
    for srm in ("no", "yes"):
        m, sd = _model(CA, srm)
        with torch.no_grad():
            lg = m(x).numpy()
        out[f"logits_{srm}"] = lg
        p_ref = _envelopes(R, sd, x, srm, lg, out)
        print(srm, "20x224 probs", np.round(p_ref.ravel(), 5), out[f"env_prob_{srm}_fp16"], out[f"env_prob_{srm}_bf16"],
              "logits", lg.ravel(), "env_logit", out[f"env_logit_{srm}_fp16"], out[f"env_logit_{srm}_bf16"])
    np.savez_compressed(OUT / "ca_s3d_golden_20x224.npz", **out)


if __name__ == "__main__":
    sys.path.insert(0, str(REF))
    from CA_S3D import CA_S3D_v3 as _CA  # the reference module (imports SRM/ and new_model/ beside it)
    torch.set_num_threads(16)
    if "--harness-shape" in sys.argv:
        harness_shape(_CA)
    else:
        blocks(_CA)
