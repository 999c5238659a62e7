"""Write tests/golden/conv_stack_envelope.json: the gate of the fused stem's
random-operand test (tests/test_conv_stack_gpu.py), measured on the CPU against
the reference and never against the kernel.

Three chained convs with two intermediate 16-bit roundings have no useful
worst-case bound in bf16: one intermediate value that rounds the other way
because of the fp32 summation order moves every output under it.  So, on the
very operands the GPU test uses (tests/conv_stack_ref.py::stem_random_operands,
same seeds), per dtype and input path:

  envelope   stem_ref accumulated in float32 against stem_ref accumulated in
             float64: "ulp", the largest difference in 16-bit ulps of
             max(|ref|, rms/2) (the unit of test_gpu_parity._ulp_diff), and
             "flips", the fraction of outputs that differ at all.  The GPU test
             allows 2 x each against the float64 reference: the kernel's
             bias-first fp32 order is a third order of the same kind.
  mutants    that the gate can fail: the float64 chain with conv2's tap (1, 2)
             dropped, and with conv1's out-of-image pixels left at relu(b1)
             instead of 0, each against the float64 reference.  "ratio" is the
             mutant's ulp figure over the gate's (2 x envelope); it must be at
             least 10 (if not, the operands change, not the gate).
             "flips_ratio" is recorded for information (the border mutant touches
             only the outermost pixels).

Runs on the CPU, reads nothing outside the repository.
"""
from __future__ import annotations

import json
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(REPO / "tests"))

import torch  # noqa: E402

import conv_stack_ref as R  # noqa: E402

OUT = REPO / "tests" / "golden" / "conv_stack_envelope.json"
MARGIN = 2.0
MUTANTS = ("drop_tap", "pad_relu_b1")


def measure():
    res = {"margin": MARGIN, "n": R.STEM_RANDOM_N, "seed": R.STEM_RANDOM_SEED}
    for dt in ("fp16", "bf16"):
        res[dt] = {}
        for path, u8 in (("u8", True), ("f32", False)):
            ops = R.stem_random_operands(dt, u8)
            ref = R.stem_ref(*ops, dt, u8, acc=torch.float64)
            ulp, flips = R.ulp_diff_and_flips(R.stem_ref(*ops, dt, u8, acc=torch.float32), ref, dt)
            entry = {"ulp": ulp, "flips": flips, "mutants": {}}
            for m in MUTANTS:
                mu, mf = R.ulp_diff_and_flips(R.stem_ref(*ops, dt, u8, acc=torch.float64, mutant=m), ref, dt)
                entry["mutants"][m] = {"ratio": round(mu / (MARGIN * ulp), 1),
                                       "flips_ratio": round(mf / (MARGIN * flips), 2)}
            res[dt][path] = entry
            print(dt, path, json.dumps(entry))
    return res


def main():
    torch.manual_seed(0)
    res = measure()
    bad = [(dt, p, m, e["mutants"][m]["ratio"]) for dt in ("fp16", "bf16") for p, e in res[dt].items()
           for m in MUTANTS if e["mutants"][m]["ratio"] < 10]
    if bad:
        raise SystemExit(f"mutants within 10x of the gate: {bad}")
    OUT.write_text(json.dumps(res, indent=1) + "\n")
    print(f"wrote {OUT}")


if __name__ == "__main__":
    main()
