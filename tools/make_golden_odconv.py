"""Generate the fixtures of cvit_GGCA_ADD_ODConv and cvit_GGCA_ODConv
(fac_fake_amd/odconv.py) under tests/golden/ from the REFERENCE's own class code.

Needs the reference checkout (``--reference DIR`` or $FAC_REFERENCE_DIR: the
directory that holds ``CViT-main/``), so it runs only where that exists.  Like
tools/make_golden_scconv.py it parses ``CViT-main/model/other/<name>.py`` with
``ast`` and executes its imports, assignments, functions and class definitions
unchanged, on the CPU, with a stub for the absent ``torchsummary``.

The fixtures are data only (no reference source), on make_odconv_state_dict(name,
0) and 8 make_crops crops (seed 41, slots 0..7):

  odconv_keys.json          {class: the reference state_dict's keys and shapes, in order}
  odconv_block_golden.npz   "<kind>/<shape>": the reference's own ODConv2d(c, c,
                            3, padding=1) module in fp32 on a small signed
                            ("signed") and a post-ReLU ("relu") input per width,
                            with the generator's weights (block_case), and
                            "<kind>/<shape>/att": ca | fa | sa | ka from the
                            module's own attention(x)
  odconv_golden.npz         per class "<class>/logits", "/probs": its fp32
                            outputs on the 8 crops; per ODConv site its input and
                            output map ("<class>/features1.13_in_sum",
                            "_sample", ...): the float64 sum and every 997th value
  odconv_envelope.json      per class and dtype the largest probability
                            difference between the golden and
                            tests/odconv_ref.py's 16-bit emulation over the 8
                            crops; "fp32": forward_fp32's largest logit distance
                            from the reference class; "blocks": per site the
                            figures asserted below and the across-crop spread of
                            ka (recorded, not asserted)

It asserts (the gains and tables at weights.ODCONV_GAIN are what to adjust;
``--calibrate`` prints the four tables, measured block by block on the reference
classes):
  * odconv_ref.odconv_block in float64 is the reference module (in float64) to
    1e-12 on the block cases, attentions included;
  * on the fixture crops, at every site: the float64 restatement's output and
    attentions are the reference module's own (hooked, fp32) to 1e-5 of the
    largest output and 2e-6; no ka entry exceeds 0.9 and every
    kernel has ka >= 0.05 on some crop; the 5th to 95th percentiles of ca and of
    fa span at least 0.25 .. 0.75; sa has an entry below 0.4 and one above 0.6;
    ||out|| / ||in|| of the reference module's output after BatchNorm and ReLU
    (the bare site: of the raw output) lies in 0.25 .. 4;
  * no golden probability within 0.05 of 0 or 1.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
from pathlib import Path

sys.dont_write_bytecode = True
REPO = Path(__file__).resolve().parents[1]
OUT = REPO / "tests" / "golden"
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(REPO / "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import odconv_ref as R  # noqa: E402
from fac_fake_amd import weights as W  # noqa: E402
from fac_fake_amd.weights import _odconv_specs, make_crops, make_odconv_state_dict, synthetic_state_dict, uniform  # noqa: E402
from tools.make_golden import ref_normalize  # noqa: E402
from tools.make_golden_bfm import load_reference_class  # noqa: E402
from tools.make_golden_other import _summ  # noqa: E402

NAMES = R.NAMES
CROP_SEED = 41
N_CROPS = 8
MARGIN = 0.05
N_KEYS = {NAMES[0]: 269, NAMES[1]: 217}
BLOCK_SHAPES = [(2, 64, 10, 14), (3, 128, 6, 6), (1, 256, 4, 18)]
BLOCK_KINDS = ("signed", "relu")


def block_case(shape, kind):
    """(state_dict of an ODConv2d(c, c, 3) under prefix "od", x NCHW fp32) of one
    recorded block case; every crop has its own per-channel offset, so the pooled
    means, and with them the attentions, differ between the crops."""
    n, c, h, w = shape
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in synthetic_state_dict(_odconv_specs("od", c), 0).items()}
    tag = f"{kind}/{c}x{h}x{w}"
    x = torch.from_numpy(uniform("odconv_block_x/" + tag, n * c * h * w, 0).reshape(n, c, h, w).copy()) * 2.5
    x = x + 1.5 * torch.from_numpy(uniform("odconv_block_off/" + tag, n * c, 0).reshape(n, c, 1, 1).copy())
    return sd, (torch.relu(x + 0.5) if kind == "relu" else x)


def block_key(shape, kind):
    return kind + "/" + "x".join(map(str, shape))


def _load_block(ODConv2d, sd, c, dtype):
    mod = ODConv2d(c, c, kernel_size=3, stride=1, padding=1).to(dtype).eval()
    mod.load_state_dict({k[len("od."):]: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()})
    return mod


def _att_of(mod, x):
    ca, fa, sa, ka = mod.attention(x)
    B = x.shape[0]
    return torch.cat([ca.reshape(B, -1), fa.reshape(B, -1), sa.reshape(B, -1), ka.reshape(B, -1)], 1)


def _site_module(m, p):
    return m.odconv if p == "odconv" else m.features1[int(p.split(".")[1])]


def _run(cls, name, sd, x):
    m = cls(image_size=224, patch_size=7, num_classes=2, channels=512, dim=1024, depth=6, heads=8, mlp_dim=2048).eval()
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    got = {}
    for p, *_ in R.SITES[name]:
        _site_module(m, p).register_forward_hook(
            lambda _m, i, o, p=p: got.update({p + "_in": i[0].detach().clone(), p + "_raw": o.detach().clone()}))
    with torch.no_grad():
        logits = m(x)
    return m, logits, got


def _r4(v):
    return float(f"{float(v):.4g}")


def calibrate(classes, x):
    for name in NAMES[::-1]:               # the bare odconv first: cvit_GGCA_ADD_ODConv holds its draw unused
        for p, bn, _c, _h, _pool in R.SITES[name]:
            _m, _lg, got = _run(classes[name], name, make_odconv_state_dict(name, 0), x)
            fc = torch.from_numpy(make_odconv_state_dict(name, 0)[p + ".attention.fc.weight"]).flatten(1).double()
            z = got[p + "_in"].double().mean((2, 3)) @ fc.t()
            W.ODCONV_FC_MEAN[p], W.ODCONV_FC_STD[p] = _r4(z.mean()), _r4(z.std())
            print(p, "fc p mean", W.ODCONV_FC_MEAN[p], "std", W.ODCONV_FC_STD[p], flush=True)
            if bn is not None:
                _m, _lg, got = _run(classes[name], name, make_odconv_state_dict(name, 0), x)
                raw = got[p + "_raw"].double()
                W.ODCONV_OUT_STD[bn], W.ODCONV_OUT_MEAN[bn] = _r4(raw.std()), _r4(raw.mean())
                print(bn, "std", W.ODCONV_OUT_STD[bn], "mean", W.ODCONV_OUT_MEAN[bn], flush=True)
    for k in ("ODCONV_FC_MEAN", "ODCONV_FC_STD", "ODCONV_OUT_STD", "ODCONV_OUT_MEAN"):
        print(k, "=", getattr(W, k))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("FAC_REFERENCE_DIR"), required="FAC_REFERENCE_DIR" not in os.environ,
                    help="the directory that holds the reference's CViT-main/")
    ap.add_argument("--dry-run", action="store_true", help="print the figures, write nothing")
    ap.add_argument("--calibrate", action="store_true",
                    help="measure the ODCONV_FC_* and ODCONV_OUT_* tables block by block, print them, write nothing")
    args = ap.parse_args(argv)
    torch.manual_seed(0)
    torch.set_num_threads(16)
    x = ref_normalize(make_crops(N_CROPS, seed=CROP_SEED))
    classes = {name: load_reference_class(Path(args.reference), name) for name in NAMES}
    ODConv2d = classes[NAMES[0]].__init__.__globals__["ODConv2d"]

    if args.calibrate:
        calibrate(classes, x)
        return

    gold_b = {}
    for shape in BLOCK_SHAPES:
        for kind in BLOCK_KINDS:
            sd, xb = block_case(shape, kind)
            c = shape[1]
            with torch.no_grad():
                m32, m64 = _load_block(ODConv2d, sd, c, torch.float32), _load_block(ODConv2d, sd, c, torch.float64)
                want32, want64 = m32(xb), m64(xb.double())
                att32, att64 = _att_of(m32, xb), _att_of(m64, xb.double())
                got64, parts = R.odconv_block(xb, R.odconv_fold(sd, "od", None, torch.float64), torch.float64, parts=True, raw=True)
            d64 = float((got64 - want64).abs().max())
            da = float((R.att_row(parts) - att64).abs().max())
            ka = parts["ka"]
            print(f"ODConv {shape} {kind}: float64 restatement vs module {d64:.3e} (attentions {da:.3e}); fp32 module vs float64 "
                  f"module {float((want32.double() - want64).abs().max()):.3e} at values up to {float(want64.abs().max()):.3e}; "
                  f"argmax ka per crop {ka.argmax(1).tolist()}", flush=True)
            assert d64 <= 1e-12 * max(1.0, float(want64.abs().max())) and da <= 1e-12, (shape, kind, d64, da)
            gold_b[block_key(shape, kind)] = want32.numpy()
            gold_b[block_key(shape, kind) + "/att"] = att32.numpy()

    keys, gold, env = {}, {"crop_seed": np.int64(CROP_SEED)}, {}
    for name in NAMES:
        sd = make_odconv_state_dict(name, 0)
        m, logits, got = _run(classes[name], name, sd, x)
        keys[name] = [[k, list(v.shape)] for k, v in m.state_dict().items()]
        assert len(keys[name]) == N_KEYS[name], len(keys[name])
        p_ref = torch.sigmoid(logits)
        print(name, "logits", logits.numpy().tolist(), "probs", p_ref.numpy().tolist(), flush=True)
        gold[name + "/logits"], gold[name + "/probs"] = logits.numpy(), p_ref.numpy()
        out32, maps = R.forward_fp32(name, sd, x, return_features=True)
        e = env[name] = {"fp32": float((out32 - logits).abs().max()), "blocks": {}}
        sdt = {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}
        for p, bn, c, _h, _pool in R.SITES[name]:
            f = got[p + "_in"]
            _summ(gold, f"{name}/{p}_in", f)
            _summ(gold, f"{name}/{p}", maps[p])
            ops = R.odconv_fold(sdt, p, bn)
            mod_raw = got[p + "_raw"]                     # the reference module's own output at the site
            with torch.no_grad():
                raw, att = R.odconv_block(f, ops, torch.float64, parts=True, raw=True)
                mod_att = _att_of(_site_module(m, p), f).double()
                post = mod_raw * ops["scale"].view(1, -1, 1, 1) + ops["shift"].view(1, -1, 1, 1)
                post = torch.relu(post) if bn is not None else post
            ca, fa, sa, ka = att["ca"], att["fa"], att["sa"], att["ka"]
            ratio = float(post.norm() / f.norm())         # of the reference's output, after the BatchNorm and ReLU
            d_mod = float((raw - mod_raw.double()).abs().max())
            d_att = float((R.att_row(att) - mod_att).abs().max())
            # the restatement's attentions and output are the fp32 module's at this site, at fp32 accuracy
            assert d_mod <= 1e-5 * float(mod_raw.abs().max()) and d_att <= 2e-6, (p, d_mod, d_att)
            q = lambda t: (float(torch.quantile(t.flatten(), 0.05)), float(torch.quantile(t.flatten(), 0.95)))  # noqa: E731
            rec = {"ka_max": float(ka.max()), "ka_best_per_kernel": ka.max(0).values.tolist(), "ca_q05_q95": q(ca), "fa_q05_q95": q(fa),
                   "sa_min": float(sa.min()), "sa_max": float(sa.max()), "ratio": ratio,
                   "ka_spread_across_crops": float((ka.max(0).values - ka.min(0).values).max()),
                   "ca_spread_across_crops": float((ca.max(0).values - ca.min(0).values).max())}
            print(f"{name} {p}: {rec}; raw output std {float(raw.std()):.4g} mean {float(raw.mean()):.4g}; float64 restatement vs fp32 "
                  f"module {d_mod:.3e} at values up to {float(mod_raw.abs().max()):.3e}, attentions {d_att:.3e}", flush=True)
            assert rec["ka_max"] <= 0.9 and min(rec["ka_best_per_kernel"]) >= 0.05, (p, rec)
            assert rec["ca_q05_q95"][0] <= 0.25 and rec["ca_q05_q95"][1] >= 0.75, (p, rec)
            assert rec["fa_q05_q95"][0] <= 0.25 and rec["fa_q05_q95"][1] >= 0.75, (p, rec)
            assert rec["sa_min"] < 0.4 and rec["sa_max"] > 0.6, (p, rec)
            assert 0.25 <= ratio <= 4, (p, ratio)
            e["blocks"][p] = rec
        assert float(p_ref.min()) >= MARGIN and float(p_ref.max()) <= 1 - MARGIN, "a golden probability is saturated"
        for dt in ("fp16", "bf16"):
            e[dt] = float((torch.sigmoid(R.forward_emulated(name, sd, x, dtype=dt)) - p_ref).abs().max())
        print(name, "envelope", e, flush=True)
    if args.dry_run:
        return
    (OUT / "odconv_keys.json").write_text(json.dumps(keys))
    np.savez_compressed(OUT / "odconv_block_golden.npz", **gold_b)
    np.savez_compressed(OUT / "odconv_golden.npz", **gold)
    (OUT / "odconv_envelope.json").write_text(json.dumps(env, indent=1))


if __name__ == "__main__":
    main()
